// sg_paths.h — the host interface between the C ABI (siamese_hip.hip, sg_embed.hip) and
// the pair paths: sg_generic.hip (path 0), sg_fast.hip with its Attention translation unit
// sg_fast_att.hip (path 1), sg_fast32.hip (path 2) and sg_web.hip (path 3).  Every function
// that crosses a translation unit is declared here, once, and every file that defines or
// calls one includes this header.  Host code only.
//
// Who validates what: the ABI layer checks counts, pointers, the model (sg_build_plan and
// the *_supported / *_lds_ok queries) and which path may take a device seed, a class table,
// an Adam step or a store source, in the order include/siamese_hip.h documents, before it
// fills an SgPairRun.  A launcher checks only what its own kernel needs (the 32-bit pair
// index range, the store's shape against its record capacity, the NTN buffer) and ignores
// the fields its path does not serve.
#pragma once
#include "sg_plan.h"

// device properties (siamese_hip.hip)
int sg_num_cus();

// One launch of a pair path: forward (s_out) or forward + backward into the gradient slab
// (one row of n_params + 1 floats per workgroup, *blocks_out rows).  The default is the null
// case of every member.
struct SgPairRun {
  bool bwd = false;
  const void *recs = nullptr;                 // packed pair records, or
  const sg_pair_source_t *src = nullptr;      // the dense graph store they are gathered from
  const int32_t *order = nullptr;             // processing order (sg_pair_order)
  const int32_t *class_start = nullptr;       // class table of the order (sg_fast)
  int64_t n_pairs = 0;
  int64_t pair_offset = 0;
  int64_t batch_total = 0;
  const float *params = nullptr;
  uint64_t seed = 0;
  const uint64_t *seed_dev = nullptr;         // dropout seed in device memory (sg_fast)
  const float *y_stats = nullptr;
  float *s_out = nullptr;
  float *slab = nullptr;
  float *ntn = nullptr;                       // per-pair NTN-gradient buffer
  const SgAdamPre *adam_pre = nullptr;        // sg_train_step's step scalars (sg_fast)
  hipStream_t stream = nullptr;
};

// ---- launch shape of the kernels that run the generic LDS stack ----
// sg_generic_kernel (sg_generic.hip) and sg_embed_nodes_kernel (sg_embed_nodes.hip, every
// embed-once call on single graphs): a workgroup holds an optional gradient accumulator and
// one slice of P.wave_floats per wavefront, and each wavefront walks the call's units (pairs
// of graphs).
constexpr size_t kSgGenLdsAim = 81920u;     // 80 KB: four waves shrink until the workgroup fits
constexpr size_t kSgGenLdsMax = 163840u;    // 160 KB, a CU's LDS: larger workgroups are refused
constexpr size_t kSgLdsNoAttr = 65536u;     // 64 KB: dynamic LDS above it needs the attribute
constexpr int kSgGenMaxPerCu = 8;           // workgroups per CU the launch counts on, 1 .. 8

struct SgGenLaunch {
  int waves_per_block;
  int blocks;
  size_t lds_bytes;
  bool fits() const { return lds_bytes <= kSgGenLdsMax; }
};

// The shape for an accumulator of acc_floats floats (0: none) and `units` units: no more
// workgroups than the device holds at once, at least one.
inline SgGenLaunch sg_gen_launch_shape(const SgGenPlan &P, int acc_floats, int64_t units) {
  SgGenLaunch L;
  const size_t gbytes = (size_t)((acc_floats + 3) & ~3) * 4u;
  const size_t wbytes = (size_t)P.wave_floats * 4u;
  int nw = 4;
  while (nw > 1 && gbytes + nw * wbytes > kSgGenLdsAim) --nw;
  L.waves_per_block = nw;
  L.lds_bytes = gbytes + nw * wbytes;
  int per_cu = (int)(kSgGenLdsMax / (L.lds_bytes ? L.lds_bytes : 1u));
  per_cu = per_cu < 1 ? 1 : (per_cu > kSgGenMaxPerCu ? kSgGenMaxPerCu : per_cu);
  const int64_t want = (units + nw - 1) / nw;
  const int64_t cap = (int64_t)sg_num_cus() * per_cu;
  L.blocks = (int)(want < cap ? (want > 0 ? want : 1) : cap);
  return L;
}

// before the launch of a kernel with more dynamic LDS than the default limit
inline void sg_allow_lds(const void *kernel, size_t lds_bytes) {
  if (lds_bytes > kSgLdsNoAttr)
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

// generic path (sg_generic.hip)
int sg_generic_lds_ok(const SgGenPlan &P, bool bwd);
int64_t sg_generic_slab_floats(const SgGenPlan &P, int64_t n_pairs);
int sg_generic_run(const SgGenPlan &P, const SgPairRun &r, int *blocks_out);
// fused path (sg_fast.hip; the Attention stack's kernels are in sg_fast_att.hip)
int sg_fast_supported(const sg_model_t *m, const SgGenPlan &P);
int64_t sg_fast_slab_floats(const SgGenPlan &P, int64_t n_pairs);
int sg_fast_needs_ntn(const SgGenPlan &P);
int sg_fast_run(const sg_model_t *m, const SgGenPlan &P, const SgPairRun &r, int *blocks_out);
int sg_fast_att_run(const sg_model_t *m, const SgGenPlan &P, const SgPairRun &r,
                    int *blocks_out);
// fused capacity-32 path (sg_fast32.hip)
int sg_fast32_supported(const sg_model_t *m, const SgGenPlan &P);
int64_t sg_fast32_slab_floats(const SgGenPlan &P, int64_t n_pairs);
int64_t sg_fast32_ntn_floats(int64_t n_pairs);
int sg_fast32_run(const sg_model_t *m, const SgGenPlan &P, const SgPairRun &r, int *blocks_out);
// NTN W / V / bias gradients from a per-pair buffer (sg_fast32.hip; sg_fast's pooled stacks)
int sg_ntn_wgrad_run(const float *ntn, int64_t n_pairs, int D, int oW, int oV, int obn, int C,
                     float *slab, int blocks, hipStream_t st, bool compact);
// graph-store path for Web-sized graphs (sg_web.hip)
int sg_web_plan_params(const sg_model_t *m, int64_t *n_params);
int sg_web_lds_ok(const sg_model_t *m);
int64_t sg_web_ws_bytes(const sg_model_t *m, int64_t chunk, int64_t n_pairs);
int sg_web_release_aux();
int sg_web_run(const sg_model_t *m, const sg_csr_store_t *store, const int32_t *pairs,
               const float *labels, int64_t n_pairs, int64_t pair_offset, int64_t batch_total,
               const float *params, uint64_t seed, const float *y_stats, int add_label,
               float *s_out, float *grad_out, float *loss_out, void *workspace, int64_t chunk,
               bool bwd, hipStream_t st);
// the NTN head of a path-3 model for the embed-once score grid (sg_web_grid.hip):
// parameter offsets and head options; SG_OK only for a model sg_model_validate puts on path 3
struct SgWebHead {
  int D, Dp, K;
  int oW, oV, oU, obn;   // obn = -1: no bias
  int ntn_mode, final_act;
  float yeta;
};
int sg_web_head_plan(const sg_model_t *m, SgWebHead *H);

// ---- layer shapes the fused kernels are written for ----
constexpr int kSgH1 = 32, kSgH2 = 16, kSgK = 10;   // GCN widths, NTN feature maps

// Sparse GCN(d_in → 32, relu) → GCN(32 → 16, identity), both with bias
inline bool sg_gcn_prefix_shape(const sg_model_t *m) {
  const sg_layer_t *Ly = m->layers;
  return Ly[0].kind == SG_GCN && Ly[0].sparse_inputs && Ly[0].output_dim == kSgH1 &&
         Ly[0].act == SG_ACT_RELU && Ly[0].bias &&
         Ly[1].kind == SG_GCN && Ly[1].input_dim == kSgH1 && Ly[1].output_dim == kSgH2 &&
         Ly[1].act == SG_ACT_IDENTITY && Ly[1].bias;
}

// an NTN(D, K = 10, relu, bias) head
inline bool sg_ntn_head_shape(const sg_layer_t &L, int D) {
  return L.kind == SG_NTN && L.input_dim == D && L.output_dim == kSgK &&
         L.act == SG_ACT_RELU && L.bias;
}

// The reference's default stack (config.py:44-66): the GCN prefix → Dense(16 → 1, relu) →
// Padding(D, 0) → NTN(D), Gaussian final activation, d_in <= 32 (two 16-row type tiles for
// the one-hot gW0 MFMA).  Returns the Padding / NTN dimension D, or 0.
inline int sg_default_stack_dim(const sg_model_t *m) {
  if (m->num_layers != 5 || !sg_gcn_prefix_shape(m)) return 0;
  const sg_layer_t *Ly = m->layers;
  if (Ly[2].kind != SG_DENSE || Ly[2].input_dim != kSgH2 || Ly[2].output_dim != 1 ||
      Ly[2].act != SG_ACT_RELU || !Ly[2].bias)
    return 0;
  if (Ly[3].kind != SG_PADDING || Ly[3].padding_value != 0.f) return 0;
  const int D = Ly[3].output_dim;
  if (D <= 0 || !sg_ntn_head_shape(Ly[4], D)) return 0;
  if (m->final_act != SG_FINAL_GAUSSIAN || m->d_in > 32) return 0;
  return D;
}

// ---- kernel arguments the fused launchers fill alike ----
// The fields FastArgs (sg_fast.hip) and F32Args (sg_fast32.hip) share by name and by
// expression.  ntn_layer is the NTN's index in model.layers, dense whether layer 2 is the
// Dense layer (the pooled stacks have none: its keep probability is 1, its offsets -1).
template <class Args>
void sg_fill_pair_args(Args &A, const sg_model_t *m, const SgGenPlan &P, const SgPairRun &r,
                       int ntn_layer, bool dense, int shared_floats, int wave_floats) {
  const sg_pair_source_t *src = r.src;
  A.recs = (const uint8_t *)r.recs;
  A.src_store = src ? 1 : 0;
  A.G = src ? src->n_graphs : 0;
  A.sadj = src ? (decltype(A.sadj))src->adj : nullptr;
  A.stypes = src ? (decltype(A.stypes))src->types : nullptr;
  A.sn = src ? src->n : nullptr;
  A.spairs = src ? src->pair_idx : nullptr;
  A.grid_base = src ? src->grid_base : 0;
  A.slabels = src ? src->labels : nullptr;
  A.status = src ? src->status : nullptr;
  A.order = r.order;
  A.n_pairs = r.n_pairs;
  A.pair_offset = r.pair_offset;
  A.rw4h = P.hbm_words / 4;
  A.rec_bf16 = P.adj_dtype == SG_DTYPE_BF16 ? 1 : 0;
  A.params = r.params;
  A.y_stats = r.y_stats;
  A.s_out = r.s_out;
  A.slab = r.slab;
  A.ntn = r.ntn;
  A.key = sg_seed_key(r.seed);
  const float keep = m->keep_prob;
  const float k0 = m->layers[0].dropout ? keep : 1.f, k1 = m->layers[1].dropout ? keep : 1.f;
  const float k2 = (dense && m->layers[2].dropout) ? keep : 1.f;
  const float k4 = m->layers[ntn_layer].dropout ? keep : 1.f;
  A.thr0 = sg_keep_threshold(k0);
  A.thr1 = sg_keep_threshold(k1);
  A.thr2 = sg_keep_threshold(k2);
  A.thr4 = sg_keep_threshold(k4);
  A.ik0 = 1.f / k0;
  A.ik1 = 1.f / k1;
  A.ik2 = 1.f / k2;
  A.ik4 = 1.f / k4;
  A.yeta = m->yeta;
  A.inv_batch = r.batch_total > 0 ? 1.f / (float)r.batch_total : 0.f;
  A.d_in = P.d_in;
  A.n_params = P.n_params;
  A.shared_floats = shared_floats;
  A.wave_floats = wave_floats;
  A.oW0 = P.L[0].offW;
  A.ob0 = P.L[0].offB;
  A.oW1 = P.L[1].offW;
  A.ob1 = P.L[1].offB;
  A.oWd = dense ? P.L[2].offW : -1;
  A.obd = dense ? P.L[2].offB : -1;
  A.oW = P.offW;
  A.oV = P.offV;
  A.oU = P.offU;
  A.obn = P.offB;
}

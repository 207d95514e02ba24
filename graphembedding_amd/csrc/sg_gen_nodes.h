// sg_gen_nodes.h — forward and backward of the generic node-level stack (GCN / Dense /
// Padding / Average / Attention) for the two graphs a wavefront holds in its LDS slice.
// Shared by the generic pair kernel (sg_generic.hip) and the embedding kernel
// (sg_embed_nodes.hip), so a graph's embedding and its gradient are computed by the code that
// scores and trains its pairs.
//
// Reference math: layers.py:91-118 (GCN), 136-140 (Average), 154-160 (Attention),
// 192-205 (Dense), 223-227 (Padding), 332-338 (sparse dropout).
#pragma once
#include "sg_plan.h"

static __device__ __forceinline__ int rows_of(int fixed, int n) { return fixed < 0 ? n : fixed; }

// ---------------------------------------------------------------------------
// Forward of the node-level stack for both graphs of the pair at once.
// Tensors are [2][R][d] row-major; rows >= rows_s are zero.
// ---------------------------------------------------------------------------
static __device__ void gen_forward_nodes(const SgGenPlan &P, float *S,
                                         const float *__restrict__ prm, const float *adj,
                                         const int *types, int n0, int n1, uint32_t pk,
                                         int lane) {
  const int nmax = P.n_max;
  for (int l = 0; l < P.nl; ++l) {
    const SgGenLayer &L = P.L[l];
    const int r0 = rows_of(L.rin_fixed, n0), r1 = rows_of(L.rin_fixed, n1);
    const float *x = L.l_in >= 0 ? S + L.l_in : nullptr;
    float *out = S + L.l_out;
    if (L.kind == SG_GCN || L.kind == SG_DENSE) {
      float *xd = S + L.l_xd;
      float *pre = S + L.l_pre;
      float *tmp = S + P.l_tmp;
      const int din = L.din, dout = L.dout, R = L.Rin;
      // (1) dropout of the input (layers.py:97-100, 196)
      if (L.sparse) {
        for (int e = lane; e < 2 * nmax; e += SG_WAVE) {
          const int s = e / nmax, n = e - s * nmax;
          const int rs = s ? r1 : r0;
          xd[e] = (n < rs && sg_keep(pk, L.li, s, n, L.thr)) ? L.inv_keep : 0.f;
        }
      } else {
        for (int e = lane; e < 2 * R * din; e += SG_WAVE) {
          const int s = e / (R * din), rem = e - s * R * din, r = rem / din;
          const int rs = s ? r1 : r0;
          float v = 0.f;
          if (r < rs && sg_keep(pk, L.li, s, rem, L.thr)) v = x[e] * L.inv_keep;
          xd[e] = v;
        }
      }
      sg_wsync();
      // (2) xd · W  (row gather of W for the one-hot X, layers.py:106-107)
      float *dst = (L.kind == SG_GCN) ? tmp : pre;
      for (int e = lane; e < 2 * R * dout; e += SG_WAVE) {
        const int s = e / (R * dout), rem = e - s * R * dout, r = rem / dout, j = rem - r * dout;
        const int rs = s ? r1 : r0;
        float acc = 0.f;
        if (r < rs) {
          if (L.sparse) {
            int t = types[s * nmax + r];
            t = t < 0 ? 0 : (t >= din ? din - 1 : t);
            acc = xd[s * nmax + r] * prm[L.offW + t * dout + j];
          } else {
            const float *xr = xd + (s * R + r) * din;
            for (int i = 0; i < din; ++i) acc = fmaf(xr[i], prm[L.offW + i * dout + j], acc);
          }
          if (L.kind == SG_DENSE && L.bias) acc += prm[L.offB + j];
        }
        dst[e] = acc;
      }
      sg_wsync();
      // (3) GCN: Â · (xd W) + b  (layers.py:110-116)
      if (L.kind == SG_GCN) {
        for (int e = lane; e < 2 * R * dout; e += SG_WAVE) {
          const int s = e / (R * dout), rem = e - s * R * dout, n = rem / dout, j = rem - n * dout;
          const int rs = s ? r1 : r0;
          float acc = 0.f;
          if (n < rs) {
            const float *ar = adj + (s * nmax + n) * nmax;
            const float *tc = tmp + s * R * dout + j;
            for (int m = 0; m < rs; ++m) acc = fmaf(ar[m], tc[m * dout], acc);
            if (L.bias) acc += prm[L.offB + j];
          }
          pre[e] = acc;
        }
        sg_wsync();
      }
      for (int e = lane; e < 2 * R * dout; e += SG_WAVE) {
        const int s = e / (R * dout), r = (e - s * R * dout) / dout;
        const int rs = s ? r1 : r0;
        out[e] = r < rs ? sg_act(L.act, pre[e]) : 0.f;
      }
      sg_wsync();
    } else if (L.kind == SG_PADDING) {
      const int d = L.din, Pr = L.Rout, Rin = L.Rin;
      for (int e = lane; e < 2 * Pr * d; e += SG_WAVE) {
        const int s = e / (Pr * d), rem = e - s * Pr * d, r = rem / d, c = rem - r * d;
        const int rs = s ? r1 : r0;
        out[e] = (r < rs && r < Rin) ? x[(s * Rin + r) * d + c] : L.padv;
      }
      sg_wsync();
    } else if (L.kind == SG_AVERAGE) {
      const int d = L.din, Rin = L.Rin;
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, c = e - s * d;
        const int rs = s ? r1 : r0;
        float acc = 0.f;
        for (int r = 0; r < rs; ++r) acc += x[(s * Rin + r) * d + c];
        out[e] = acc / (float)rs;
      }
      sg_wsync();
    } else {  // SG_ATTENTION (layers.py:154-160)
      const int d = L.din, Rin = L.Rin;
      float *temp = S + L.l_temp, *hv = S + L.l_hv, *att = S + L.l_att;
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, c = e - s * d;
        const int rs = s ? r1 : r0;
        float acc = 0.f;
        for (int r = 0; r < rs; ++r) acc += x[(s * Rin + r) * d + c];
        temp[e] = acc / (float)rs;
      }
      sg_wsync();
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, c = e - s * d;
        float acc = 0.f;
        for (int i = 0; i < d; ++i) acc = fmaf(temp[s * d + i], prm[L.offW + i * d + c], acc);
        hv[e] = tanhf(acc);
      }
      sg_wsync();
      for (int e = lane; e < 2 * Rin; e += SG_WAVE) {
        const int s = e / Rin, r = e - s * Rin;
        const int rs = s ? r1 : r0;
        float v = 0.f;
        if (r < rs) {
          float acc = 0.f;
          for (int c = 0; c < d; ++c) acc = fmaf(x[(s * Rin + r) * d + c], hv[s * d + c], acc);
          v = 1.f / (1.f + expf(-acc));
        }
        att[e] = v;
      }
      sg_wsync();
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, c = e - s * d;
        const int rs = s ? r1 : r0;
        float acc = 0.f;
        for (int r = 0; r < rs; ++r) acc = fmaf(att[s * Rin + r], x[(s * Rin + r) * d + c], acc);
        out[e] = acc;
      }
      sg_wsync();
    }
  }
}

namespace {

// ---------------------------------------------------------------------------
// Backward of the node-level stack; gin = gradient of the last layer's output.
// Parameter gradients go to the workgroup accumulator G with LDS atomics.
// ---------------------------------------------------------------------------
__device__ void gen_backward_nodes(const SgGenPlan &P, float *S, float *G,
                                   const float *__restrict__ prm, const float *adj,
                                   const int *types, int n0, int n1, uint32_t pk, int lane,
                                   float *gcur, float *gnext) {
  const int nmax = P.n_max;
  for (int l = P.nl - 1; l >= 0; --l) {
    const SgGenLayer &L = P.L[l];
    const int r0 = rows_of(L.rin_fixed, n0), r1 = rows_of(L.rin_fixed, n1);
    const float *x = L.l_in >= 0 ? S + L.l_in : nullptr;
    if (L.kind == SG_GCN || L.kind == SG_DENSE) {
      const int din = L.din, dout = L.dout, R = L.Rin;
      const float *xd = S + L.l_xd, *pre = S + L.l_pre, *out = S + L.l_out;
      float *gpre = S + P.l_tmp;
      float *gsup = S + P.l_tmp2;
      for (int e = lane; e < 2 * R * dout; e += SG_WAVE) {
        const int s = e / (R * dout), r = (e - s * R * dout) / dout;
        const int rs = s ? r1 : r0;
        gpre[e] = r < rs ? sg_act_grad(L.act, pre[e], out[e], gcur[e]) : 0.f;
      }
      sg_wsync();
      if (L.bias) {
        for (int j = lane; j < dout; j += SG_WAVE) {
          float acc = 0.f;
          for (int sr = 0; sr < 2 * R; ++sr) acc += gpre[sr * dout + j];
          atomicAdd(&G[L.offB + j], acc);
        }
      }
      const float *gz = gpre;  // gradient w.r.t. (xd · W)
      if (L.kind == SG_GCN) {
        // adjoint of the sparse matmul: gsup = Âᵀ gpre
        for (int e = lane; e < 2 * R * dout; e += SG_WAVE) {
          const int s = e / (R * dout), rem = e - s * R * dout, m = rem / dout, j = rem - m * dout;
          const int rs = s ? r1 : r0;
          float acc = 0.f;
          if (m < rs) {
            const float *ac = adj + s * nmax * nmax + m;
            const float *gc = gpre + s * R * dout + j;
            for (int n = 0; n < rs; ++n) acc = fmaf(ac[n * nmax], gc[n * dout], acc);
          }
          gsup[e] = acc;
        }
        sg_wsync();
        gz = gsup;
      }
      if (L.sparse) {
        // scatter-add into the rows of W0 selected by the node types
        const float *xm = xd;
        for (int e = lane; e < 2 * nmax * dout; e += SG_WAVE) {
          const int s = e / (nmax * dout), rem = e - s * nmax * dout, n = rem / dout, j = rem - n * dout;
          const int rs = s ? r1 : r0;
          const float sc = xm[s * nmax + n];
          if (n < rs && sc != 0.f) {
            int t = types[s * nmax + n];
            t = t < 0 ? 0 : (t >= din ? din - 1 : t);
            atomicAdd(&G[L.offW + t * dout + j], sc * gz[e]);
          }
        }
      } else {
        for (int e = lane; e < din * dout; e += SG_WAVE) {
          const int i = e / dout, j = e - i * dout;
          float acc = 0.f;
          for (int sr = 0; sr < 2 * R; ++sr) acc = fmaf(xd[sr * din + i], gz[sr * dout + j], acc);
          atomicAdd(&G[L.offW + e], acc);
        }
        for (int e = lane; e < 2 * R * din; e += SG_WAVE) {
          const int s = e / (R * din), rem = e - s * R * din, r = rem / din, i = rem - r * din;
          const int rs = s ? r1 : r0;
          float v = 0.f;
          if (r < rs && sg_keep(pk, L.li, s, rem, L.thr)) {
            const float *gr = gz + (s * R + r) * dout;
            float acc = 0.f;
            for (int j = 0; j < dout; ++j) acc = fmaf(gr[j], prm[L.offW + i * dout + j], acc);
            v = acc * L.inv_keep;
          }
          gnext[e] = v;
        }
      }
      sg_wsync();
    } else if (L.kind == SG_PADDING) {
      const int d = L.din, Rin = L.Rin, Pr = L.Rout;
      for (int e = lane; e < 2 * Rin * d; e += SG_WAVE) {
        const int s = e / (Rin * d), rem = e - s * Rin * d, r = rem / d, c = rem - r * d;
        const int rs = s ? r1 : r0;
        gnext[e] = (r < rs && r < Pr) ? gcur[(s * Pr + r) * d + c] : 0.f;
      }
      sg_wsync();
    } else if (L.kind == SG_AVERAGE) {
      const int d = L.din, Rin = L.Rin;
      for (int e = lane; e < 2 * Rin * d; e += SG_WAVE) {
        const int s = e / (Rin * d), rem = e - s * Rin * d, r = rem / d, c = rem - r * d;
        const int rs = s ? r1 : r0;
        gnext[e] = r < rs ? gcur[s * d + c] / (float)rs : 0.f;
      }
      sg_wsync();
    } else {  // SG_ATTENTION
      const int d = L.din, Rin = L.Rin;
      const float *temp = S + L.l_temp, *hv = S + L.l_hv, *att = S + L.l_att;
      float *gzb = S + L.l_gz, *gu = S + L.l_gu, *gt = S + L.l_gt;
      for (int e = lane; e < 2 * Rin; e += SG_WAVE) {
        const int s = e / Rin, r = e - s * Rin;
        const int rs = s ? r1 : r0;
        float v = 0.f;
        if (r < rs) {
          float ga = 0.f;
          for (int c = 0; c < d; ++c) ga = fmaf(gcur[s * d + c], x[(s * Rin + r) * d + c], ga);
          v = ga * att[e] * (1.f - att[e]);
        }
        gzb[e] = v;
      }
      sg_wsync();
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, c = e - s * d;
        const int rs = s ? r1 : r0;
        float gh = 0.f;
        for (int r = 0; r < rs; ++r) gh = fmaf(gzb[s * Rin + r], x[(s * Rin + r) * d + c], gh);
        gu[e] = gh * (1.f - hv[e] * hv[e]);
      }
      sg_wsync();
      for (int e = lane; e < d * d; e += SG_WAVE) {
        const int i = e / d, c = e - i * d;
        atomicAdd(&G[L.offW + e], temp[i] * gu[c] + temp[d + i] * gu[d + c]);
      }
      for (int e = lane; e < 2 * d; e += SG_WAVE) {
        const int s = e / d, i = e - s * d;
        float acc = 0.f;
        for (int c = 0; c < d; ++c) acc = fmaf(gu[s * d + c], prm[L.offW + i * d + c], acc);
        gt[e] = acc;
      }
      sg_wsync();
      for (int e = lane; e < 2 * Rin * d; e += SG_WAVE) {
        const int s = e / (Rin * d), rem = e - s * Rin * d, r = rem / d, c = rem - r * d;
        const int rs = s ? r1 : r0;
        gnext[e] = r < rs ? att[s * Rin + r] * gcur[s * d + c] + gzb[s * Rin + r] * hv[s * d + c] +
                                gt[s * d + c] / (float)rs
                          : 0.f;
      }
      sg_wsync();
    }
    float *t = gcur;
    gcur = gnext;
    gnext = t;
  }
}

}  // namespace

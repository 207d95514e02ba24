"""Compare two scripts/isa_dump.py output directories (parent tree, new tree) for the merge
of the four node-stack kernels into sg_embed_nodes_kernel<BWD, MASK>:
- the units that must not move: whole .norm files;
- the kernels that stay in sg_embed.hip / sg_embed_train.hip: kernel by kernel (instruction
  stream with block labels renumbered per kernel, .amdhsa_ lines, resource .set lines);
- the four instantiations against the kernels they replace: registers, scratch, spills (from
  the .s files' metadata) and instruction counts.
Usage: python cmp_isa.py PARENT_DIR NEW_DIR [KERNEL_SUBSTRING_TO_PRINT_THE_DIFF_OF]"""
import difflib
import hashlib
import os
import re
import subprocess
import sys

A, B = sys.argv[1], sys.argv[2]
FIXED = ['siamese_hip', 'sg_generic', 'sg_fast', 'sg_fast_att', 'sg_fast32', 'sg_sampler',
         'sg_web', 'sg_search']
REPLACED = {   # parent (unit, kernel) -> instantiation of sg_embed_nodes_kernel
    ('sg_embed', 'sg_embed_kernel'): '<false, false>',
    ('sg_embed_train', 'sg_embed_bwd_kernel'): '<true, false>',
    ('sg_embed_drop', 'sg_embed_drop_kernel'): '<false, true>',
    ('sg_embed_drop', 'sg_embed_drop_bwd_kernel'): '<true, true>',
}
ok = True
for u in FIXED:
    pa, pb = (open(os.path.join(d, u + '.hip.s.norm'), 'rb').read() for d in (A, B))
    print(hashlib.sha1(pb).hexdigest(), u + '.hip.s.norm', 'identical' if pa == pb else 'DIFFERS')
    ok &= pa == pb


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), text=True,
                         capture_output=True).stdout.split('\n')
    return dict(zip(names, out))


def canon(name):
    n = name.replace('(anonymous namespace)::', '')
    n = re.sub(r'^void ', '', n)
    n = re.sub(r'\(bool\)1', 'true', n)
    n = re.sub(r'\(bool\)0', 'false', n)
    return re.sub(r'\(.*$', '', n)   # drop the parameter list


def kernels(d, unit):
    """canonical name -> (instruction lines, .amdhsa_ and resource .set lines)"""
    body, hsa = {}, {}
    cur = hk = None
    for ln in open(os.path.join(d, unit + '.hip.s.norm')).read().split('\n'):
        m = re.match(r'^(_Z\w+):\s*$', ln)
        if m and not m.group(1).endswith('.kd'):
            cur = m.group(1)
            body[cur] = []
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            cur, hk = None, m.group(1)
            hsa[hk] = []
            continue
        if re.match(r'^\s*\.end_amdhsa_kernel', ln):
            hk = None
            continue
        if hk and re.match(r'^\s*\.amdhsa_', ln):
            hsa[hk].append(ln.strip())
            continue
        m = re.match(r'^\s*\.set (_Z\w+)\.(\w+), (.*)$', ln)
        if m and m.group(1) in hsa:
            hsa[m.group(1)].append('.set %s %s' % (m.group(2), m.group(3).replace(m.group(1), 'KERNEL')))
            continue
        if cur is not None:
            body[cur].append(re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip()))
    dm = demangle(list(body))
    res = {}
    for sym, b in body.items():
        if sym not in hsa:
            continue
        seen = {}
        ren = lambda m: seen.setdefault(m.group(0), '.L%d' % len(seen))
        txt = [re.sub(r'\.LBB_\d+', ren, l.replace(sym, 'KERNEL')) for l in b]
        res[canon(dm[sym])] = (txt, hsa[sym])
    return res


def meta(d, unit):
    """canonical name -> {vgpr, agpr, scratch, sgpr_spill, vgpr_spill} from the .s metadata"""
    txt = open(os.path.join(d, unit + '.hip.s')).read()
    res = {}
    for blk in txt.split('  - .agpr_count:')[1:]:
        blk = '.agpr_count:' + blk
        f = lambda k: re.search(r'\.%s:\s*(\S+)' % k, blk).group(1)
        res[f('name')] = dict(vgpr=int(f('vgpr_count')), agpr=int(f('agpr_count')),
                              scratch=int(f('private_segment_fixed_size')),
                              sgpr_spill=int(f('sgpr_spill_count')),
                              vgpr_spill=int(f('vgpr_spill_count')))
    dm = demangle(list(res))
    return {canon(dm[k]): v for k, v in res.items()}


for unit in ('sg_embed', 'sg_embed_train'):
    P, N = kernels(A, unit), kernels(B, unit)
    for k in sorted(set(P) | set(N)):
        if (unit, k) in REPLACED:
            continue
        if k not in P or k not in N:
            print('ONE SIDE ONLY', unit, k)
            ok = False
        elif P[k] == N[k]:
            print('identical', unit, k, len(P[k][0]), 'lines')
        else:
            ok = False
            d = [l for l in difflib.unified_diff(P[k][0], N[k][0], lineterm='', n=0)
                 if not l.startswith(('---', '+++', '@@'))]
            print('DIFFERS  ', unit, k, len(d), 'stream diff lines of', len(P[k][0]))
print('ALL IDENTICAL' if ok else 'DIFFERENCES')

NK, NM = kernels(B, 'sg_embed_nodes'), meta(B, 'sg_embed_nodes')
insn = lambda lines: sum(1 for l in lines if re.match(r'^\s+[a-z]\w+', l) and not l.lstrip().startswith('.'))
for (unit, k), inst in REPLACED.items():
    pm, nm = meta(A, unit)[k], NM['sg_embed_nodes_kernel' + inst]
    pk, nk = kernels(A, unit)[k], NK['sg_embed_nodes_kernel' + inst]
    # sg_mix is two v_mul_u32_u24: more of them than in the parent's kernel is mask code
    muls = lambda lines: sum(1 for l in lines if 'v_mul_u32_u24' in l)
    print('%-26s -> %-15s parent %s, %d instructions, %d v_mul_u32_u24 | new %s, %d instructions, '
          '%d v_mul_u32_u24' % (k, inst, pm, insn(pk[0]), muls(pk[0]), nm, insn(nk[0]), muls(nk[0])))
    if len(sys.argv) > 3 and sys.argv[3] in k:
        print('\n'.join(l for l in difflib.unified_diff(pk[0], nk[0], lineterm='', n=0)
                        if not l.startswith(('---', '+++', '@@'))))

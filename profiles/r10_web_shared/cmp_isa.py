"""Compare two scripts/isa_dump.py output directories (parent tree, new tree): every dump
but sg_web's whole, sg_web's kernel by kernel after mapping the renamed symbols (instruction
stream with block labels renumbered per kernel, .amdhsa_ lines and the resource .set lines).
Usage: python cmp_isa.py PARENT_DIR NEW_DIR [KERNEL_SUBSTRING_TO_PRINT_THE_DIFF_OF]"""
import difflib
import os
import re
import subprocess
import sys

A, B = sys.argv[1], sys.argv[2]
ok = True
for f in sorted(os.listdir(A)):
    if not f.endswith('.norm') or f == 'sg_web.hip.s.norm':
        continue
    # __hip_cuid_<hash> hashes the source's path, which differs between the two checkouts
    rd = lambda p: re.sub(rb'__hip_cuid_[0-9a-f]+', b'__hip_cuid_X', open(p, 'rb').read())
    same = rd(os.path.join(A, f)) == rd(os.path.join(B, f))
    print(f, 'identical' if same else 'DIFFERS')
    ok &= same


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), text=True,
                         capture_output=True).stdout.split('\n')
    return dict(zip(names, out))


def kernels(path):
    """symbol -> (body lines, amdhsa lines)"""
    lines = open(path).read().split('\n')
    body, hsa = {}, {}
    cur = hk = None
    for ln in lines:
        m = re.match(r'^(_Z\w+):\s*$', ln)
        if m and not m.group(1).endswith('.kd'):
            cur = m.group(1)
            body[cur] = []
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            cur = None
            hk = m.group(1)
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
            hsa[m.group(1)].append('.set %s %s' % (m.group(2), m.group(3)))
            continue
        if cur is not None:
            body[cur].append(re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip()))
    return body, hsa


def canon(name):
    n = name.replace('(anonymous namespace)::', '')
    n = re.sub(r'^void ', '', n)
    n = re.sub(r'web_gcn_kernel<\((bool\))?(\w+), (\d+), \(bool\)0>|web_gcn_kernel<(\w+), (\d+), false>',
               lambda m: 'web_gcn_kernel<%s, %s>' % (m.group(2) or m.group(4), m.group(3) or m.group(5)), n)
    n = n.replace('web_t_kernel_b3<true>', 'web_t_kernel_b3')
    n = re.sub(r'web_head_kernel<(\w+), true>', r'web_head_kernel<\1>', n)
    n = n.replace('web_gx1_kernel_b3', 'web_gx_kernel_b3<false>')
    n = n.replace('web_gx2_kernel_b3', 'web_gx_kernel_b3<true>')
    n = re.sub(r'\(bool\)1', 'true', n)
    n = re.sub(r'\(bool\)0', 'false', n)
    n = re.sub(r'\(.*$', '', n)   # drop the parameter list
    return n


def load(d):
    body, hsa = kernels(os.path.join(d, 'sg_web.hip.s.norm'))
    dm = demangle(list(body))
    res = {}
    for sym, b in body.items():
        if sym not in hsa:
            continue
        # replace every occurrence of own symbol (labels, relocs) by a placeholder
        txt = [l.replace(sym, 'KERNEL') for l in b]
        # block labels renumbered in order of first appearance: one inserted or removed
        # block must not make every later label differ
        seen = {}
        ren = lambda m: seen.setdefault(m.group(0), '.L%d' % len(seen))
        txt = [re.sub(r'\.LBB_\d+', ren, l) for l in txt]
        # trim trailing directives after the code (section switches for the descriptor)
        res[canon(dm[sym])] = (txt, hsa[sym], dm[sym])
    return res


P, N = load(A), load(B)
for k in sorted(set(P) | set(N)):
    if k not in N:
        print('GONE     ', P[k][2])
        continue
    if k not in P:
        print('NEW      ', N[k][2])
        ok = False
        continue
    pb, ph, _ = P[k]
    nb, nh, _ = N[k]
    if pb == nb and ph == nh:
        print('identical', k, len(pb), 'lines')
    else:
        ok = False
        d = [l for l in difflib.unified_diff(pb, nb, lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]
        dh = [l for l in difflib.unified_diff(ph, nh, lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]
        print('DIFFERS  ', k, 'stream diff lines', len(d), 'of', len(pb), '; amdhsa diff', dh)
        if len(sys.argv) > 3 and sys.argv[3] in k:
            print('\n'.join(d[:200]))
print('ALL IDENTICAL' if ok else 'DIFFERENCES')

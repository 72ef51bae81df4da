#!/usr/bin/env python3
"""tools/isa_stats.py <asm.s> <kernel-substring> [--loops]: register/LDS usage of a kernel and its MFMA loops.
tools/isa_stats.py --compare <a.s> <a_resource_usage.txt> <b.s> <b_resource_usage.txt> <name-regex>: the kernels of two `make asm`
outputs against each other (DESIGN.md sections 8l, 8q).  Kernels whose name (k_...) matches the regex are the ones a change may
touch: each must be identical or keep its multiset of vector, memory and LDS opcodes (register copies, v_mov_*, aside), its
VGPRs, LDS and occupancy, with no scratch and no spill; every other kernel must be identical.  Identical: the same
instructions up to s_endpgm, labels renumbered.  Exit status 1 if a kernel misses that."""
import collections
import re
import sys

KERNEL = re.compile(r'^(_Z\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel', re.S | re.M)


def base_name(mangled):
    m = re.search(r'(\d+)k_', mangled)  # <length>k_name, perhaps with the 1 of an anonymous namespace's _N_1 in front
    for d in reversed(range(len(m.group(1)) if m else 0)):
        end = m.end(1) + int(m.group(1)[d:])
        if mangled[end:end + 1] in ('I', 'E'):
            return mangled[m.end(1):end]
    return mangled


def instructions(body):
    out = []
    for line in body.split('s_endpgm')[0].split('\n'):
        line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0]).strip()
        if line and not line.startswith('.') or line.startswith('.LBB_'):
            out.append(line)
    return out


def resources(path):
    res, name = {}, None
    for line in open(path):
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2)
            res[name] = {}
        elif name:
            res[name][m.group(1)] = m.group(2)
    return res


def compare(asm_a, res_a, asm_b, res_b, pattern):
    ka = {m.group(1): instructions(m.group(2)) for m in KERNEL.finditer(open(asm_a).read())}
    kb = {m.group(1): instructions(m.group(2)) for m in KERNEL.finditer(open(asm_b).read())}
    ra, rb = resources(res_a), resources(res_b)
    print(f'kernels: {len(ka)} and {len(kb)}; only in one: {sorted(set(ka) ^ set(kb))}')
    bad = len(set(ka) ^ set(kb))
    fam = collections.defaultdict(lambda: collections.defaultdict(list))
    vec = re.compile(r'^(v_|ds_|global_|flat_|buffer_|scratch_)')
    for k in sorted(set(ka) & set(kb)):
        name, same = base_name(k), ka[k] == kb[k]
        if not re.fullmatch(pattern, name):
            if not same:
                bad += 1
                print('CHANGED outside the pattern:', k)
            fam['(others)']['identical' if same else 'CHANGED'].append(1)
            continue
        f = fam[name]
        f['identical' if same else 'changed'].append(1)
        ops = [collections.Counter(re.sub(r'_e(32|64)$', '', i.split()[0]) for i in v if vec.match(i) and not i.startswith('v_mov_')) for v in (ka[k], kb[k])]
        keys = ('VGPRs', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]', 'ScratchSize [bytes/lane]', 'SGPRs Spill', 'VGPRs Spill')
        keeps = ops[0] == ops[1] and all(ra[k][x] == rb[k][x] for x in keys) and all(rb[k][x] == '0' for x in keys[3:])
        if not keeps:
            bad += 1
            print('MISSES:', k, 'more', dict(ops[1] - ops[0]), 'fewer', dict(ops[0] - ops[1]), [(x, ra[k][x], rb[k][x]) for x in keys if ra[k][x] != rb[k][x]])
        f['sgpr'].append(int(rb[k]['TotalSGPRs']) - int(ra[k]['TotalSGPRs']))
        f['count'].append(len(kb[k]) - len(ka[k]))
        f['len'].append(len(ka[k]))
        f['vgpr'].append(int(rb[k]['VGPRs']))
        f['occ'].append(int(rb[k]['Occupancy [waves/SIMD]']))
    for name, f in sorted(fam.items()):
        if name == '(others)':
            print(f"{name}: identical {len(f['identical'])}, changed {len(f['CHANGED'])}")
            continue
        print(f"{name}: {len(f['len'])} instances, identical {len(f['identical'])}; instructions {min(f['len'])}..{max(f['len'])}, step "
              f"{min(f['count']):+d}..{max(f['count']):+d}; SGPRs step {min(f['sgpr']):+d}..{max(f['sgpr']):+d}; VGPRs {min(f['vgpr'])}..{max(f['vgpr'])}; "
              f"occupancy {min(f['occ'])}..{max(f['occ'])}")
    print('verdict:', 'ok' if not bad else f'{bad} kernels miss the rule')
    return 1 if bad else 0


if sys.argv[1] == '--compare':
    sys.exit(compare(*sys.argv[2:7]))
s = open(sys.argv[1]).read()
pat = sys.argv[2]
for m in KERNEL.finditer(s):
    if pat not in m.group(1):
        continue
    body = m.group(2)
    print(m.group(1))
    for key in ['next_free_vgpr', 'next_free_sgpr', 'accum_offset', 'group_segment_fixed_size', 'private_segment_fixed_size']:
        for l in body.split('\n'):
            if key in l:
                print('  ', l.strip())
    print('   mfma', body.count('v_mfma'), 'accvgpr', body.count('v_accvgpr'), 'scratch', body.count('scratch_'), 'lines', body.count('\n'))
    if '--loops' in sys.argv:
        lines = body.split('\n')
        for i, l in enumerate(lines):
            if 'Inner Loop Header' in l and any('v_mfma' in x for x in lines[i:i + 40]):
                j = i
                while j < len(lines) and 's_cbranch' not in lines[j]:
                    j += 1
                print('\n'.join(lines[i - 1:j + 1]))
                print('-----')

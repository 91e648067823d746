#!/usr/bin/env python3
"""Static instruction counts of ONE box step of mega_bvh_kernel, from the listing of a device-only compile:

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o k.s mort_amd/csrc/hip/mort_hip.hip
    scripts/box_step_isa.py k.s [mangled kernel name]

The step is the innermost loop that issues the node's eight ds_read_b128; it is counted from that loop's header to the
lane-count check (the first s_bcnt1_i32_b64 after it) that decides whether the wave takes another step.  Also prints
what the code object states for the kernel: registers, spilled registers, private bytes.
"""
import re, sys
txt = open(sys.argv[1]).read().split('\n')
name = sys.argv[2] if len(sys.argv) > 2 else '_Z15mega_bvh_kernelILi1024ELb0ELb0ELb0EEv8FastArgs'
a = next(i for i, l in enumerate(txt) if l.startswith(name + ':'))
b = next(i for i in range(a, len(txt)) if txt[i].startswith('.Lfunc_end'))
L = txt[a:b]
found = False
for h in [i for i, l in enumerate(L) if 'This Inner Loop Header' in l]:
    e = next((i for i in range(h, len(L)) if 's_bcnt1_i32_b64' in L[i]), len(L))
    seg = L[h:e]
    if sum('ds_read_b128' in l for l in seg) < 8:
        continue
    c = lambda pat: sum(1 for l in seg if re.match(pat, l))
    print('box step: valu %d (v_min/v_max_f32 %d, v_mov %d)  ds %d  salu %d  scratch %d' % (
        c(r'\s+v_'), c(r'\s+v_(min|max)_f32'), c(r'\s+v_mov_b'), c(r'\s+ds_'), c(r'\s+s_'), c(r'\s+scratch_')))
    found = True
    break
if not found:
    sys.exit('no loop with eight ds_read_b128 in ' + name)
meta = next(i for i, l in enumerate(txt) if re.match(r'\s+\.name:\s+' + re.escape(name) + r'\s*$', l))
for l in txt[meta:meta + 40]:
    m = re.match(r'\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)', l)
    if m:
        print('%s %s' % m.groups())

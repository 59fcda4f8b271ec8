#!/usr/bin/env python3
"""Reads the rocprofv3 --kernel-trace database of a tools/wino4f_probe.py run: per shape (12 operator calls each, in the probe's order) the
median duration of the input transform, the batched GEMM and the output transform, with the transforms' HBM rate.
usage: wino4f_trace.py results.db B [B ...]   (the probe's batch sizes, same order)
       wino4f_trace.py forms results.db MANIFEST   (a `wino4f_probe.py forms MANIFEST` run: the output transform alone, one line per form
                                                    and shape -- see the probe's docstring)"""
import json
import sqlite3
import statistics
import sys


def forms_table(db, manifest_path):
    manifest = json.load(open(manifest_path))
    rows = sqlite3.connect(db).execute("select start, end, name from kernels order by start").fetchall()
    durs = [(e - s) / 1e3 for s, e, name in rows if 'wino4f_output' in name]
    assert len(durs) == len(manifest), (len(durs), len(manifest))
    lines, order = {}, []
    for d, (B, C, name, mb, variant, rnd) in zip(durs, manifest):
        key = (B, C, name)
        if key not in lines:
            lines[key] = (mb, {})
            order.append(key)
        if rnd >= 0:
            lines[key][1].setdefault(variant, {}).setdefault(rnd, []).append(d)
    print('# us per launch alone on the device (kernel trace): median over rounds of the round medians; spread = (max - min) / median of the round')
    print('# medians, the worst variant of the line; gain = form1 against form0 (the parent commit\'s kernel, kept as the oracle); x bare = time /')
    print('# (bare transform [form1, plain, no bias] of the same shape x MB moved / bare MB); the last columns: timing ablations of form1')
    for key in order:
        B, C, name = key
        mb, var = lines[key]
        rmed = {v: [statistics.median(r) for r in rounds.values()] for v, rounds in var.items()}
        med = {v: statistics.median(r) for v, r in rmed.items()}
        spread = max((max(r) - min(r)) / statistics.median(r) for r in rmed.values())
        bmb, bvar = lines[(B, C, 'bare')]
        scaled = statistics.median([statistics.median(r) for r in bvar['form1'].values()]) * mb / bmb
        gain = 100 * (1 - med['form1'] / med['form0'])
        line = 'B=%2d C=%3d %-22s %6.1f MB  form0 %6.1f us  form1 %6.1f us  gain %+5.1f %%  spread %4.1f %%  %4.2f TB/s  x bare %4.2f -> %4.2f' % (
            B, C, name, mb, med['form0'], med['form1'], gain, 100 * spread, mb / med['form1'], med['form0'] / scaled, med['form1'] / scaled)
        line += ''.join('  | %s %6.1f' % (v, med[v]) for v in med if v not in ('form0', 'form1'))
        print(line)


if len(sys.argv) > 1 and sys.argv[1] == 'forms':
    forms_table(sys.argv[2], sys.argv[3])
    sys.exit(0)

SHAPES = [(512, 512), (256, 512), (512, 256), (256, 256), (128, 256), (256, 128), (128, 128)]
db, batches = sys.argv[1], [int(a) for a in sys.argv[2:]]
rows = sqlite3.connect(db).execute("select start, end, name, grid_x / workgroup_x from kernels order by start").fetchall()
calls, cur = [], None
for s, e, name, gx in rows:
    d = (e - s) / 1e3
    if 'wino_weight_all_kernel' in name:
        cur = {}
        calls.append(cur)
    elif cur is not None:
        for key in ('wino4f_input', 'igemm_conv_kernel', 'wino4f_output'):
            if key in name and key not in cur:
                cur[key] = (d, gx, name.split('wino4f_')[-1].split('(')[0] if 'wino4f' in name else '')
calls = [c for c in calls if len(c) == 3]
assert len(calls) == 12 * len(SHAPES) * len(batches), len(calls)
tot_in = tot_out = 0.0
for i, B in enumerate(batches):
    for j, (cin, cout) in enumerate(SHAPES):
        grp = calls[(i * len(SHAPES) + j) * 12 + 2:(i * len(SHAPES) + j + 1) * 12]
        t_in = statistics.median(c['wino4f_input'][0] for c in grp)
        t_g = statistics.median(c['igemm_conv_kernel'][0] for c in grp)
        t_out = statistics.median(c['wino4f_output'][0] for c in grp)
        px = B * 576 * 4.0
        mb_in, mb_out = px * cin * 3.25 / 1e6, px * cout * 3.25 / 1e6       # x + 2.25 x (V)  /  2.25 y (Mt) + y
        tot_in += t_in; tot_out += t_out
        print('B=%2d %3d->%3d  input %-22s %4d blocks %6.1f us %4.1f TB/s | gemm %6.1f us | output %-22s %4d blocks %6.1f us %4.1f TB/s'
              % (B, cin, cout, grp[0]['wino4f_input'][2], grp[0]['wino4f_input'][1], t_in, mb_in / t_in, t_g,
                 grp[0]['wino4f_output'][2], grp[0]['wino4f_output'][1], t_out, mb_out / t_out))
print('sum of medians: input %.1f us, output %.1f us' % (tot_in, tot_out))

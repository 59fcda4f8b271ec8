"""What the wide-row bf16 stem (plan option stem_bf16 = 2, 10..13 input channels) costs against the generic kernels a
default plan launches for such an input: one JSON line, also written to profiles/<tag>_wide_stem_rate.json.

    python tools/wide_stem_rate.py [--reps 20] [--tag r13]

Every figure is HIP events around `reps` back-to-back launches after two warm-up launches.  The forms of a row are timed alternately in
one process, two windows each, and every row is taken twice ("runs"): the difference between the runs is the spread a difference
between the forms has to exceed before it means anything.  There is no pass or fail threshold on these times.
  stem_fwd      simq_conv2d_fwd (fp32 NHWC in, fp32 out: the gather kernel a default plan launches at Cin = 10) against
                simq_conv2d_fwd_stem_bf16_wide and _wide_x16, Cin = 10, B = 32 and 128 (the wide operators prepare their 87 KB weight
                layout in the same call)
  stem_wgrad    simq_conv2d_wgrad (fp32, zeroes dW itself) against simq_conv2d_wgrad_stem_bf16_wide and _wide_x16 on a bf16 dy
  step          sample + one full plain-bf16 TD step, Cin 10, Cout 1, B = 128: a default plan on an fp32 ring, a stem_bf16 = 2 plan on the
                same ring, and a stem_bf16 = 2 + bf16_states plan on a bf16 ring
Each of the two GPU steps ("stem", "step") runs in a child process of its own under its own time limit; the parent never touches the
GPU and stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))

W, CIN = 96, 10
STEP_LIMITS = {'stem': 240, 'step': 420}          # seconds per child


def timed(launch, reps):
    import torch
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(row, forms, reps):
    """forms: [(name, launch)], timed in turn, two windows each -- the mean of each form's two windows, and every form over the first."""
    times = {name: [] for name, _ in forms}
    for _ in range(2):
        for name, launch in forms:
            times[name].append(timed(launch, reps))
    base = forms[0][0]
    for name, _ in forms:
        row[name + '_ms'] = round(sum(times[name]) / 2, 5)
    for name, _ in forms[1:]:
        row[name + '_over_' + base] = round(row[name + '_ms'] / row[base + '_ms'], 3)
    return row


def stem_rows(reps):
    import numpy as np
    import torch
    from simq import _lib as L
    from simq.fcn import to_bf16
    rows = []
    for B in (32, 128):
        rng = np.random.RandomState(B)
        x = torch.from_numpy(rng.rand(B, W, W, CIN).astype(np.float32)).cuda()
        x16 = to_bf16(x)
        w = torch.from_numpy((rng.randn(64, 7, 7, CIN) * 0.1).astype(np.float32)).cuda()
        y32 = torch.empty((B, 48, 48, 64), dtype=torch.float32, device='cuda')
        y16 = torch.empty((B, 48, 48, 64), dtype=torch.bfloat16, device='cuda')
        wl = torch.empty(int(L.lib.c.simq_conv2d_fwd_stem_bf16_wide_scratch_bytes()), dtype=torch.uint8, device='cuda')
        st = L.stream_ptr()
        generic = lambda: L.lib.call('simq_conv2d_fwd', L.ptr(x), L.ptr(w), None, L.ptr(y32), B, W, W, CIN, 64, 7, 7, 2, 3, None, st)
        wide = lambda entry, xin: (lambda: L.lib.call(entry, L.ptr(xin), L.ptr(w), L.ptr(y16), B, W, W, CIN, None, L.ptr(wl), st))
        rows.append(alternate({'op': 'stem_fwd', 'B': B, 'cin': CIN}, [('generic_f32', generic), ('wide', wide('simq_conv2d_fwd_stem_bf16_wide', x)),
                                                                      ('wide_x16', wide('simq_conv2d_fwd_stem_bf16_wide_x16', x16))], reps))
        dy32 = torch.randn((B, 48, 48, 64), device='cuda')
        dy16 = dy32.to(torch.bfloat16)
        dw = torch.empty((64, 7, 7, CIN), dtype=torch.float32, device='cuda')
        slabs = L.lib.c.simq_conv2d_wgrad_stem_bf16_slabs(B, W, W, CIN, -1)
        part = torch.empty(slabs * 64 * 49 * CIN, dtype=torch.float32, device='cuda')
        generic_wg = lambda: L.lib.call('simq_conv2d_wgrad', L.ptr(x), L.ptr(dy32), L.ptr(dw), B, W, W, CIN, 64, 7, 7, 2, 3, st)
        wide_wg = lambda entry, xin: (lambda: L.lib.call(entry, L.ptr(xin), L.ptr(dy16), L.ptr(dw), B, W, W, CIN, L.ptr(part), st))
        rows.append(alternate({'op': 'stem_wgrad', 'B': B, 'cin': CIN, 'slabs': slabs},
                              [('generic_f32', generic_wg), ('wide', wide_wg('simq_conv2d_wgrad_stem_bf16_wide', x)),
                               ('wide_x16', wide_wg('simq_conv2d_wgrad_stem_bf16_wide_x16', x16))], reps))
    return rows


def step_rows(reps):
    import torch
    import simq as S
    import simq.learner as sl
    from simq import synth
    cout, B, n = 1, 128, 512
    gamma, lr, momentum, weight_decay, clip = 0.75, 0.01, 0.9, 1e-4, 100          # (the base configuration's: train.py:186)
    trs = synth.make_transitions(n, CIN, cout, 5, terminal_frac=0.1)
    rings = {}
    for dtype in ('fp32', 'bf16'):
        rings[dtype] = S.DeviceReplayBuffer(n, CIN, dtype=dtype)
        for t in trs:
            rings[dtype].push(*t)
    torch.cuda.synchronize()
    forms = []
    for name, dtype, options in (('default_fp32_pool', 'fp32', None), ('wide_fp32_pool', 'fp32', {'stem_bf16': 2}),
                                 ('wide_bf16_pool', 'bf16', {'stem_bf16': 2, 'bf16_states': 1})):
        policy, target = S.FCN(CIN, cout, precision='bf16', options=options), S.FCN(CIN, cout, precision='bf16', options=options)
        target.copy_state_from(policy)                                           # (timing does not read values)
        policy.train(); target.eval()

        def launch(policy=policy, target=target, ring=rings[dtype]):
            sl.train_step(policy, target, ring.sample(B), gamma, B, lr, momentum, weight_decay, clip, use_double_dqn=True, sync=False)
        forms.append((name, launch))
    return [alternate({'op': 'step (sample + TD step)', 'B': B, 'cin': CIN, 'cout': cout}, forms, reps)]


def child(step, reps):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('wide_stem_rate.py needs a GPU')
    rows = stem_rows if step == 'stem' else step_rows
    print('ROWS ' + json.dumps([rows(reps), rows(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tag', default='r13')
    ap.add_argument('--step', choices=sorted(STEP_LIMITS), help='(internal) run one GPU step in this process')
    args = ap.parse_args()
    if args.step:
        return child(args.step, args.reps)
    result = {'metric': 'wide_stem', 'unit': 'ms per launch, mean of two alternating windows of `reps` launches per form', 'reps': args.reps,
              'runs': [[], []]}
    for step in ('stem', 'step'):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--reps', str(args.reps)], stdout=subprocess.PIPE,
                               text=True, timeout=STEP_LIMITS[step])
        except subprocess.TimeoutExpired:
            raise SystemExit('step %r exceeded its %d s limit: nothing further is started on the GPU' % (step, STEP_LIMITS[step]))
        if r.returncode != 0:
            raise SystemExit('step %r ended with status %d: nothing further is started on the GPU\n%s' % (step, r.returncode, r.stdout[-2000:]))
        runs = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('ROWS ')][-1][5:])
        for k in range(2):
            result['runs'][k] += runs[k]
    line = json.dumps(result)
    with open(os.path.join(ROOT, 'profiles', '%s_wide_stem_rate.json' % args.tag), 'w') as out:
        out.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()

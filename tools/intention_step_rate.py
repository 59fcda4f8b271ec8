"""What the one-call intention supervision step and its three kernels cost against what they replace: one JSON line,
also written to profiles/<tag>_intention_step_rate.json.

    python tools/intention_step_rate.py [--reps 20] [--tag r14]

The forms of a row are timed alternately in one process, two windows each, and every row is taken twice ("runs"): the difference between
the runs is the spread a difference between the forms has to exceed before it means anything.  There is no pass or fail threshold.
  kernels   HIP events around `reps` back-to-back launches after two warm-up launches, B = 32 and 128, C = 5 and 10 state channels, with the
            bytes each NEW form asks for and the rate that makes:
              split    simq_split_last_channel (fp32) against simq_intention_split fp32 -> fp32 with the target, and -- what a bf16 pool
                       ran -- simq_states_to_f32 + simq_split_last_channel against simq_intention_split bf16 -> bf16 without it
              bce      simq_bce_with_logits on a contiguous target against simq_bce_with_logits_state on the fp32 and on the bf16 state
                       (bytes: logits, gradient and one target element per pixel; the strided read sweeps the whole state, state_bytes)
              concat   simq_sigmoid_concat (fp32) against simq_sigmoid_concat_x fp32 -> fp32, and simq_states_to_f32 + simq_sigmoid_concat
                       against simq_sigmoid_concat_x bf16 -> bf16
  loop      host wall time of `iters` alternating simq.train + simq.train_intention iterations (train.py:255-261), unfused against fused:
            fp32 nets at C = 5, B = 32 on an fp32 ring; plain-bf16 nets at C = 10, B = 128 on a bf16 ring (unfused: an intention net without
            bf16_states, which widens the batch; fused: one with it).  host_ms: until the last loss is back on the host; wall_ms: until
            the device is idle; both per iteration.
Each GPU step ("kernels", "loop") runs in a child process of its own under its own time limit; the parent never touches the GPU and
stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))

W = 96
STEP_LIMITS = {'kernels': 300, 'loop': 540}          # seconds per child


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


def alternate(row, forms, reps, bytes_of=None):
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
    for name, nbytes in (bytes_of or {}).items():
        row[name + '_bytes'] = int(nbytes)
        row[name + '_GBps'] = round(nbytes / (row[name + '_ms'] * 1e-3) / 1e9, 1)
    return row


def kernel_rows(reps):
    import numpy as np
    import torch
    from simq import _lib as L
    from simq.fcn import to_bf16
    call, ptr, rows = L.lib.call, L.ptr, []
    for B in (32, 128):
        for C in (5, 10):
            P = B * W * W
            rng = np.random.RandomState(B + C)
            x32 = torch.from_numpy(rng.rand(P, C).astype(np.float32)).cuda()
            x16 = to_bf16(x32)
            wide = torch.empty_like(x32)
            head32, head16 = torch.empty(P, C - 1, device='cuda'), torch.empty(P, C - 1, dtype=torch.bfloat16, device='cuda')
            last = torch.empty(P, device='cuda')
            st = L.stream_ptr()
            old32 = lambda: call('simq_split_last_channel', ptr(x32), ptr(head32), ptr(last), P, C, st)

            def old16():
                call('simq_states_to_f32', ptr(x16), ptr(wide), P * C, st)
                call('simq_split_last_channel', ptr(wide), ptr(head32), ptr(last), P, C, st)
            new32 = lambda: call('simq_intention_split', ptr(x32), 0, ptr(head32), 0, ptr(last), P, C, st)
            new16 = lambda: call('simq_intention_split', ptr(x16), 1, ptr(head16), 1, None, P, C, st)
            rows.append(alternate({'op': 'split', 'B': B, 'C': C}, [('split_last_channel_f32', old32), ('intention_split_f32', new32),
                                                                      ('to_f32_then_split', old16), ('intention_split_bf16', new16)], reps,
                                  {'intention_split_f32': P * (8 * C), 'intention_split_bf16': P * (2 * C + 2 * (C - 1))}))
            logits = torch.from_numpy((rng.randn(P) * 3).astype(np.float32)).cuda()
            target = x32[:, C - 1].contiguous()
            dx, ls = torch.empty(P, device='cuda'), torch.empty(1, dtype=torch.float64, device='cuda')
            scratch = torch.empty(int(L.lib.c.simq_bce_state_scratch_bytes()), dtype=torch.uint8, device='cuda')
            bce_old = lambda: call('simq_bce_with_logits', ptr(logits), ptr(target), P, ptr(dx), ptr(ls), st)
            bce_new = lambda x, b16: (lambda: call('simq_bce_with_logits_state', ptr(logits), ptr(x), b16, P, C, ptr(dx), ptr(ls), ptr(scratch), st))
            row = alternate({'op': 'bce', 'B': B, 'C': C}, [('bce_with_logits', bce_old), ('bce_state_f32', bce_new(x32, 0)),
                                                            ('bce_state_bf16', bce_new(x16, 1))], reps,
                            {'bce_state_f32': P * 12, 'bce_state_bf16': P * 10})
            row['state_bytes_f32'], row['state_bytes_bf16'] = P * C * 4, P * C * 2
            rows.append(row)
            Cs = C - 1
            s32 = x32[:, :Cs].contiguous()
            s16 = to_bf16(s32)
            swide = torch.empty_like(s32)
            out32, out16 = torch.empty(P, C, device='cuda'), torch.empty(P, C, dtype=torch.bfloat16, device='cuda')
            cat_old32 = lambda: call('simq_sigmoid_concat', ptr(s32), ptr(logits), ptr(out32), None, P, Cs, st)

            def cat_old16():
                call('simq_states_to_f32', ptr(s16), ptr(swide), P * Cs, st)
                call('simq_sigmoid_concat', ptr(swide), ptr(logits), ptr(out32), None, P, Cs, st)
            cat_new32 = lambda: call('simq_sigmoid_concat_x', ptr(s32), 0, ptr(logits), ptr(out32), 0, None, P, Cs, st)
            cat_new16 = lambda: call('simq_sigmoid_concat_x', ptr(s16), 1, ptr(logits), ptr(out16), 1, None, P, Cs, st)
            rows.append(alternate({'op': 'concat', 'B': B, 'C': C}, [('sigmoid_concat_f32', cat_old32), ('sigmoid_concat_x_f32', cat_new32),
                                                                       ('to_f32_then_concat', cat_old16), ('sigmoid_concat_x_bf16', cat_new16)], reps,
                                  {'sigmoid_concat_x_f32': P * (4 * Cs + 4 + 4 * C), 'sigmoid_concat_x_bf16': P * (2 * Cs + 4 + 2 * C)}))
    return rows


def loop_rows(iters):
    import types
    import torch
    import simq as S
    from simq import synth
    gamma, lr, momentum, weight_decay = 0.75, 0.01, 0.9, 1e-4                      # (the base configuration's: train.py:186)
    rows = []
    for name, C, B, precision, dtype, q_opts, i_opts in (
            ('fp32 C=5 B=32', 5, 32, 'fp32', 'fp32', None, (None, None)),
            ('bf16 pools C=10 B=128', 10, 128, 'bf16', 'bf16', {'stem_bf16': 2, 'bf16_states': 1}, (None, {'bf16_states': 1}))):
        n = 4 * B
        ring = S.DeviceReplayBuffer(n, C, dtype=dtype)
        for t in synth.make_transitions(n, C, 1, 5, terminal_frac=0.1):
            ring.push(*t)
        cfg = types.SimpleNamespace(batch_size=B, use_double_dqn=True, grad_norm_clipping=100)
        forms = {}
        for fused in (False, True):
            policy, target = S.FCN(C, 1, precision=precision, options=q_opts), S.FCN(C, 1, precision=precision, options=q_opts)
            target.copy_state_from(policy)                                         # (timing does not read values)
            policy.train(); target.eval()
            inet = S.FCN(C - 1, 1, precision=precision, options=i_opts[fused])
            inet.train()
            inet.fused_step = fused
            opt = torch.optim.SGD(policy.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
            opt_i = torch.optim.SGD(inet.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)

            def window(policy=policy, target=target, inet=inet, opt=opt, opt_i=opt_i):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    batch = ring.sample(B)
                    S.train(cfg, policy, target, opt, batch, None, gamma)
                    S.train_intention(inet, opt_i, batch, None)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                return (t1 - t0) * 1e3 / iters, (time.perf_counter() - t0) * 1e3 / iters
            forms['fused' if fused else 'unfused'] = window
        for w in forms.values():                                                   # warm-up: workspaces, streams, the allocator's pools
            w()
        times = {k: [] for k in forms}
        for _ in range(2):
            for k, w in forms.items():
                times[k].append(w())
        row = {'op': 'loop (sample + train + train_intention)', 'case': name, 'iters': iters}
        for k, v in times.items():
            row[k + '_host_ms'] = round(sum(h for h, _ in v) / 2, 4)
            row[k + '_wall_ms'] = round(sum(t for _, t in v) / 2, 4)
            row[k + '_windows_wall_ms'] = [round(t, 4) for _, t in v]
        row['fused_over_unfused_wall'] = round(row['fused_wall_ms'] / row['unfused_wall_ms'], 4)
        rows.append(row)
    return rows


def child(step, reps, iters):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('intention_step_rate.py needs a GPU')
    rows = (lambda: kernel_rows(reps)) if step == 'kernels' else (lambda: loop_rows(iters))
    print('ROWS ' + json.dumps([rows(), rows()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--tag', default='r14')
    ap.add_argument('--step', choices=sorted(STEP_LIMITS), help='(internal) run one GPU step in this process')
    args = ap.parse_args()
    if args.step:
        return child(args.step, args.reps, args.iters)
    result = {'metric': 'intention_step', 'unit': 'ms: kernels per launch (HIP events), loop per iteration (host clock); mean of two alternating '
              'windows per form', 'reps': args.reps, 'iters': args.iters, 'runs': [[], []]}
    for step in ('kernels', 'loop'):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--reps', str(args.reps), '--iters', str(args.iters)],
                               stdout=subprocess.PIPE, text=True, timeout=STEP_LIMITS[step])
        except subprocess.TimeoutExpired:
            raise SystemExit('step %r exceeded its %d s limit: nothing further is started on the GPU' % (step, STEP_LIMITS[step]))
        if r.returncode != 0:
            raise SystemExit('step %r ended with status %d: nothing further is started on the GPU\n%s' % (step, r.returncode, r.stdout[-2000:]))
        runs = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('ROWS ')][-1][5:])
        for k in range(2):
            result['runs'][k] += runs[k]
    line = json.dumps(result)
    with open(os.path.join(ROOT, 'profiles', '%s_intention_step_rate.json' % args.tag), 'w') as out:
        out.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()

"""What a replay pool of bf16 states costs and saves on the GPU, kernel by kernel: one JSON line, also written to
profiles/<tag>_bf16_states_rate.json.

    python tools/bf16_states_rate.py [--reps 20] [--tag r12]

Every figure is HIP events around `reps` back-to-back launches after two warm-up launches.  The fp32 and the bf16 form of each operator
are timed alternately in the same job, and the whole table is taken twice ("runs"): the difference between the two runs is the spread a
difference between the two forms has to exceed before it means anything.  There is no pass or fail threshold on these times.
  stem_fwd / stem_wgrad    simq_conv2d_fwd_stem_bf16 / simq_conv2d_wgrad_stem_bf16 against their _x16 forms, Cin = 5, B = 32 and 128, and Cin = 4
                           at B = 128 (even Cin: the 16-byte fragments of the bf16 form start on 4-byte boundaries, odd Cin: on odd elements)
                           (the standalone operators prepare the 58 KB weight layout in the same call: both forms pay it)
  local_state_slots        simq_local_state_images_slots against _slots_bf16 on P = 64 and 256 problems of tests/golden/local_maps_*.npz
  gather                   the two gathers of one minibatch (simq_replay_gather over states and over the non-final next states), B = 128,
                           from an fp32 ring and from a bf16 ring of the same 1 024 transitions
  step                     one full plain-bf16 TD step of BASELINE configs[2]'s shape (Cin 5, Cout 2, B = 128), sampled from an fp32 ring by
                           a default plan and from a bf16 ring by a bf16_states plan
The bytes saved per pool, per gather and per checkpoint follow from the sizes and are computed, not measured ("bytes")."""
import argparse
import ctypes
import glob
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

W = 96


def timed(launch, reps):
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


def pair(row, f32, bf16, reps):
    """Both forms, alternating: fp32, bf16, fp32, bf16 -- the mean of each form's two windows."""
    a, b = [], []
    for _ in range(2):
        a.append(timed(f32, reps))
        b.append(timed(bf16, reps))
    row.update(fp32_ms=round(sum(a) / 2, 5), bf16_ms=round(sum(b) / 2, 5))
    row['bf16_over_fp32'] = round(row['bf16_ms'] / row['fp32_ms'], 3)
    return row


def stem_rows(L, reps):
    from simq.fcn import to_bf16
    rows = []
    for B, cin in ((32, 5), (128, 5), (128, 4)):        # (Cin = 4: every fragment of the bf16 form starts on a 4-byte boundary, Cin = 5: none does)
        rng = np.random.RandomState(B)
        x = torch.from_numpy(rng.rand(B, W, W, cin).astype(np.float32)).cuda()
        x16 = to_bf16(x)
        w = torch.from_numpy((rng.randn(64, 7, 7, cin) * 0.1).astype(np.float32)).cuda()
        y = torch.empty((B, 48, 48, 64), dtype=torch.bfloat16, device='cuda')
        wl = torch.empty(58368, dtype=torch.uint8, device='cuda')
        st = L.stream_ptr()
        fwd = lambda entry, xin: (lambda: L.lib.call(entry, L.ptr(xin), L.ptr(w), L.ptr(y), B, W, W, cin, None, L.ptr(wl), st))
        rows.append(pair({'op': 'stem_fwd', 'B': B, 'cin': cin}, fwd('simq_conv2d_fwd_stem_bf16', x), fwd('simq_conv2d_fwd_stem_bf16_x16', x16), reps))
        dy = torch.randn((B, 48, 48, 64), device='cuda').to(torch.bfloat16)
        dw = torch.empty((64, 7, 7, cin), dtype=torch.float32, device='cuda')
        part = torch.empty(min(512, -(-(B * 48 * 3) // 16)) * 64 * 49 * cin, dtype=torch.float32, device='cuda')
        wg = lambda entry, xin: (lambda: L.lib.call(entry, L.ptr(xin), L.ptr(dy), L.ptr(dw), B, W, W, cin, L.ptr(part), st))
        rows.append(pair({'op': 'stem_wgrad', 'B': B, 'cin': cin}, wg('simq_conv2d_wgrad_stem_bf16', x), wg('simq_conv2d_wgrad_stem_bf16_x16', x16), reps))
    return rows


def local_state_rows(L, reps):
    import local_maps_oracle
    import test_gpu_device_transitions as tdt
    fx = local_maps_oracle.load_fixture(sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'local_maps_*.npz')))[0])
    maps, masks = tdt.device_inputs(fx)
    rows = []
    for P in (64, 256):
        t = tdt.Tables(fx, maps, masks, problems=[p % len(fx['states']) for p in range(P)])
        need = L.lib.c.simq_local_state_slots_desc_bytes(t.G, t.n_robots, t.P, t.C)
        desc = torch.empty(need, dtype=torch.uint8, device='cuda')
        slots = tdt.slots_array([int(s) for s in np.random.RandomState(P).permutation(P + 8)[:P]])
        pools = {torch.float32: torch.empty((P + 8, W, W, t.C), dtype=torch.float32, device='cuda'),
                 torch.bfloat16: torch.empty((P + 8, W, W, t.C), dtype=torch.bfloat16, device='cuda')}
        head, st = t.head(), L.stream_ptr()
        run = lambda entry, pool: (lambda: L.lib.call(entry, *head, slots, L.ptr(desc), ctypes.c_int64(need), L.ptr(pool), ctypes.c_int64(P + 8), st))
        rows.append(pair({'op': 'local_state_slots', 'P': P, 'C': t.C}, run('simq_local_state_images_slots', pools[torch.float32]),
                         run('simq_local_state_images_slots_bf16', pools[torch.bfloat16]), reps))
    return rows


def rings(S, cin, cout, n):
    from simq import synth
    out = {}
    trs = synth.make_transitions(n, cin, cout, 5, terminal_frac=0.1)
    for dtype in ('fp32', 'bf16'):
        ring = S.DeviceReplayBuffer(n, cin, dtype=dtype)
        for t in trs:
            ring.push(*t)
        out[dtype] = ring
    torch.cuda.synchronize()
    return out


def gather_row(S, L, both, reps):
    B = 128
    random.seed(1)
    idx = both['fp32'].sample_indices(B)
    launches = {}
    for dtype, ring in both.items():
        recs = [ring.buffer[i] for i in idx]
        index = torch.tensor([int(r.state) for r in recs], dtype=torch.int64, device='cuda')
        nindex = torch.tensor([int(r.next_state) for r in recs if r.next_state is not None], dtype=torch.int64, device='cuda')
        state = torch.empty((B, W, W, ring.C), dtype=ring.dtype, device='cuda')
        nstate = torch.empty((nindex.numel(), W, W, ring.C), dtype=ring.dtype, device='cuda')
        st = L.stream_ptr()

        def launch(ring=ring, index=index, nindex=nindex, state=state, nstate=nstate):
            L.lib.call('simq_replay_gather', L.ptr(ring.states), ring.item, L.ptr(index), B, L.ptr(state), st)
            L.lib.call('simq_replay_gather', L.ptr(ring.next_states), ring.item, L.ptr(nindex), nindex.numel(), L.ptr(nstate), st)
        launches[dtype] = launch
    return pair({'op': 'gather', 'B': B, 'cin': both['fp32'].C}, launches['fp32'], launches['bf16'], reps)


def step_row(S, both, reps):
    import simq.learner as sl
    cin, cout, B = 5, 2, 128
    gamma, lr, momentum, weight_decay, clip = 0.75, 0.01, 0.9, 1e-4, 100          # (the base configuration's: train.py:186)
    launches = {}
    for dtype, options in (('fp32', None), ('bf16', {'bf16_states': 1})):
        policy, target = S.FCN(cin, cout, precision='bf16', options=options), S.FCN(cin, cout, precision='bf16', options=options)
        target.copy_state_from(policy)                                           # (the reference's initialisation: timing does not read values)
        policy.train(); target.eval()
        ring = both[dtype]

        def launch(policy=policy, target=target, ring=ring):
            sl.train_step(policy, target, ring.sample(B), gamma, B, lr, momentum, weight_decay, clip, use_double_dqn=True, sync=False)
        launches[dtype] = launch
    return pair({'op': 'step (sample + TD step)', 'B': B, 'cin': cin, 'cout': cout}, launches['fp32'], launches['bf16'], reps)


def byte_counts(cin=5, capacity=10000, B=128):
    state = W * W * cin
    return {'cin': cin, 'state_bytes': {'fp32': 4 * state, 'bf16': 2 * state},
            'ring_of_%d_transitions_two_rings_bytes' % capacity: {'fp32': 2 * capacity * 4 * state, 'bf16': 2 * capacity * 2 * state},
            'gather_B%d_state_read_plus_write_bytes' % B: {'fp32': 2 * B * 4 * state, 'bf16': 2 * B * 2 * state},
            'checkpoint_device_to_host_per_observation_bytes': {'fp32': 4 * state, 'bf16': 2 * state},
            'checkpoint_file_per_observation_bytes': {'fp32': 4 * state, 'bf16': 4 * state}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tag', default='r12')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bf16_states_rate.py needs a GPU')
    import simq as S
    from simq import _lib as L
    both = rings(S, 5, 2, 1024)
    result = {'metric': 'bf16_states', 'unit': 'ms per launch (fp32 form, bf16 form), mean of two alternating windows of `reps` launches',
              'reps': args.reps, 'runs': [], 'bytes': byte_counts()}
    for _ in range(2):
        result['runs'].append(stem_rows(L, args.reps) + local_state_rows(L, args.reps) + [gather_row(S, L, both, args.reps), step_row(S, both, args.reps)])
    line = json.dumps(result)
    with open(os.path.join(ROOT, 'profiles', '%s_bf16_states_rate.json' % args.tag), 'w') as out:
        out.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()

"""GPU: the data-parallel HIP step (BASELINE configs[3] / configs[4]) -- simq.learner.train_step with a process group /
libsimq's RCCL communicator, i.e. simq_backward_onehot(phase 1 | 2) + the bucketed gradient all-reduces + identical clip/SGD on
every rank, one process per rank.

The GPU box has ONE MI355X, so the ranks are
  (a) a 1-rank "nccl" (== RCCL) group with libsimq's own communicator (simq_comm_*): the whole step is the data-parallel form of
      simq_train_step -- phases, ncclAllReduce on the communicator's stream, event fork/join;
  (b) 2 / 8 ranks that SHARE the GPU and talk over gloo (RCCL refuses two ranks on one device): the Python-sequenced form with
      torch.distributed collectives around the two backward phases.
Checked against
  * fixture G7 (tests/golden/dp_*.npz): the reference's own networks.FCN run replica by replica by oracle/gen_golden.py
    (nn.DataParallel semantics, policies.py:39: per-replica BatchNorm statistics, gradients summed, replica 0's running
    statistics kept) -- loss, td error, q_sa, TD targets, the fp64 gradient summary, rank-0 BN buffers; one case has shards
    that hold terminal transitions only;
  * size-independent properties at the per-GPU shapes of configs[3] (Cin 5, Cout 2 and 1, 64 transitions per rank, fp32) and
    configs[4] (128 per rank, bf16): the all-reduced gradient equals the sum of the shard gradients computed one after the other
    by a single process, every rank ends with bit-identical parameters, loss / td error are the global means.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import cases
from oracle import fcn as ofcn
from simq import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make_nets(simq, cin, cout, wseed, precision, dev):
    policy = simq.FCN(cin, cout, device=dev, precision=precision)
    target = simq.FCN(cin, cout, device=dev, precision=precision)
    policy.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, wseed)))
    target.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, wseed + 1000)))
    policy.train()
    target.eval()
    return policy, target


def _transitions(cin, cout, gB, dseed, terminal_frac):
    return synth.make_transitions(gB, cin, cout, dseed, terminal_frac=terminal_frac)


def _unclipped(policy):
    """flat gradient as all-reduced, before clip_grad_norm_ scaled it in place."""
    tn = float(policy._simq_opt_state.total_norm.item())
    coef = min(1.0, cases.CLIP / (tn + 1e-6))
    return policy.flat_grads.detach().double().cpu() / coef, tn


def _worker(rank, world, port, backend, use_comm, spec, out_dir, sync_bn=False):
    for p in (ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch.distributed as dist
    dev_index = rank % torch.cuda.device_count() if backend == 'nccl' else 0      # RCCL: one GPU per rank; gloo ranks share GPU 0
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import simq
        from simq import dist as sdist
        from simq.learner import Transition, assemble_batch, train_step
        cin, cout, gB, wseed, dseed, precision, tfrac, steps = spec
        trs = _transitions(cin, cout, gB, dseed, tfrac)
        lo, hi = sdist.shard_bounds(gB, world, rank)
        policy, target = _make_nets(simq, cin, cout, wseed, precision, dev)
        comm = sdist.Comm(dist.group.WORLD) if use_comm else None
        pg = None if use_comm else dist.group.WORLD
        if use_comm:
            # through the HBM ring, as bench.py --gpus N draws its shards: the gathers run on the upload stream and the target net's
            # forward on the early stream (StepOptions.early_target_forward) beside the communicator's collectives
            ring = simq.DeviceReplayBuffer(max(64, gB), cin, device=dev)
            for t in trs:
                ring.push(*t)
            shard = ring.gather(list(range(lo, hi)), allow_all_final=True)
            assert shard.ready_event is not None
        else:
            shard = assemble_batch(Transition(*zip(*trs[lo:hi])), dev, allow_all_final=True)
        gnf = sum(1 for t in trs if t[3] is not None)          # every rank sees the whole drawn minibatch: global non-final count
        out = {}
        if comm is not None:
            comm.time_waits(True)       # (bench.py's exposed-communication pass: timing events around the step's last simq_comm_wait)
        for s in range(steps):
            info = train_step(policy, target, shard, cases.GAMMA, hi - lo, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, cases.CLIP,
                              use_double_dqn=True, process_group=pg, global_batch=gB, comm=comm, sync_bn=sync_bn,
                              global_nonfinal=gnf if sync_bn else None)
            if comm is not None:
                ms = comm.last_wait_ms()
                assert 0.0 <= ms < 1e3, ms
                out['exposed_ms'] = ms
            if s == 0:
                g, tn = _unclipped(policy)
                out.update(grad=g.numpy(), total_norm=tn, loss=info['loss'], td_error=info['td_error'],
                           q_sa=policy._last['q_sa'].cpu().numpy(), y=policy._last['y'].cpu().numpy(),
                           bn=policy.bn_buffers.cpu().numpy(), params1=policy.flat_params.cpu().numpy())
        out.update(params=policy.flat_params.cpu().numpy(), momentum=policy._simq_opt_state.momentum.cpu().numpy(),
                   loss_last=info['loss'])
        if comm is not None:            # broadcast through the communicator: every rank adopts rank 0's running statistics
            bn = policy.bn_buffers.clone()
            comm.broadcast(bn, 0)
            comm.wait()
            out['bn_bcast'] = bn.cpu().numpy()
            comm.close()
        else:
            out['bn_bcast'] = sdist.broadcast_bn_buffers(policy.bn_buffers.clone(), dist.group.WORLD).cpu().numpy()
        np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), **out)
    finally:
        dist.destroy_process_group()


def _run_ranks(tmp_path, world, backend, use_comm, spec, sync_bn=False):
    ctx = mp.get_context('spawn')
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, use_comm, spec, str(tmp_path), sync_bn)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
    for p in procs:
        if p.is_alive():
            p.kill()
            pytest.fail('data-parallel rank did not finish (hang)')
        assert p.exitcode == 0, 'a data-parallel rank failed (exit code %r)' % p.exitcode
    return [np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r)) for r in range(world)]


def _reference_layout(simq, cin, cout, flat):
    """flat HIP gradient (OHWI conv weights) -> {reference key: flat tensor in the reference's OIHW order}."""
    from simq import arch
    from simq import _lib
    plan = _lib.Plan(cin, cout)
    out = {}
    t = torch.as_tensor(flat)
    for name, off, shape, kind in plan.tensors:
        n = int(np.prod(shape))
        v = t[off:off + n].view(shape)
        out[arch.PREFIX + name] = (v.permute(0, 3, 1, 2).contiguous() if len(shape) == 4 else v).reshape(-1)
    return out


def _sampled_relerr(got, g):
    """relative L2 error over the 16 sampled elements of every tensor against the fixture's fp64 summary + per-tensor norm check."""
    keys = [str(k) for k in g['grad_keys']]
    num = den = 0.0
    worst_norm = 0.0
    for i, k in enumerate(keys):
        flat = got[k].double()
        idx = torch.tensor(cases.sample_indices(flat.numel()))
        mine = flat[idx].numpy()
        num += ((mine - g['grad64'][i][1:]) ** 2).sum()
        den += (g['grad64'][i][1:] ** 2).sum()
        if g['grad64'][i][0] > 1e-3 * float(g['total_norm64']):
            worst_norm = max(worst_norm, abs(float(flat.norm()) - g['grad64'][i][0]) / g['grad64'][i][0])
    return (num / den) ** 0.5, worst_norm


DP_GOLDEN = [('dp_c5o2_b8_w1', 'nccl', True), ('dp_c5o2_b8_w2', 'gloo', False), ('dp_c5o2_b8_w8', 'gloo', False),
             ('dp_c5o1_b8_w2', 'gloo', False)]
# (round 6, suite budget: eight processes importing torch and sharing the one GPU take a minute of wall time for a B = 8 step -- the 8-rank
# fixture runs with --runslow / SIMQ_RUN_SLOW=1; the 1-, 2- and 4-rank fixtures stay in the default run)
_DP_PARAMS = [pytest.param(*c, id=c[0] + '-' + c[1], marks=[pytest.mark.slow] if c[0].endswith('_w8') else []) for c in DP_GOLDEN]


@pytest.mark.parametrize('name,backend,use_comm', _DP_PARAMS)
def test_dp_step_against_reference_replica_fixture(tmp_path, golden_dir, name, backend, use_comm):
    import simq
    case = [c for c in cases.DP_CASES if c[0] == name][0]
    _, cin, cout, gB, world, wseed, dseed = case
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    ranks = _run_ranks(tmp_path, world, backend, use_comm, (cin, cout, gB, wseed, dseed, 'fp32', 0.25, 1))
    r0 = ranks[0]
    for r in ranks[1:]:                 # identical clip + SGD everywhere: replicas stay bit-identical
        assert np.array_equal(r0['params'], r['params']) and np.array_equal(r0['grad'], r['grad'])
        assert r['loss'] == r0['loss'] and r['td_error'] == r0['td_error']
        assert np.array_equal(r0['bn_bcast'], r['bn_bcast'])
    assert np.array_equal(r0['bn_bcast'], r0['bn'])                             # rank 0's running statistics are the ones kept
    rel1 = lambda a, b: abs(a - b) / abs(b)
    assert rel1(float(r0['loss']), float(g['loss'])) < 1e-4 and rel1(float(r0['td_error']), float(g['td_error'])) < 1e-4
    q_sa, y = np.concatenate([r['q_sa'] for r in ranks]), np.concatenate([r['y'] for r in ranks])
    assert np.abs(q_sa - g['q_sa']).max() <= 1e-4 * np.abs(g['q_sa']).max()
    assert np.abs(y - g['y']).max() <= 1e-4 * np.abs(g['y']).max()
    # rank 0's BatchNorm buffers == replica 0's of the reference emulation (policy net: train-mode updates of ITS shard only)
    # (bn_buffers is [mean | var] per layer in reference state_dict order -- the order cases.bn_buffer_vector walks)
    want, got = g['bn_buffers_after'].astype(np.float64), r0['bn'].astype(np.float64)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    # all-reduced gradient vs the fp64 replica emulation (conditioning: DESIGN section 2; bar as in test_gpu_fcn.py)
    err, worst_norm = _sampled_relerr(_reference_layout(simq, cin, cout, r0['grad']), g)
    print('%s: sampled-gradient rel-L2 error %.3g (reference fp32 replicas: %.3g), worst per-tensor norm error %.3g, '
          'total norm %.6g vs %.6g' % (name, err, float(g['ref_fp32_grad_relerr']), worst_norm, float(r0['total_norm']), float(g['total_norm64'])))
    assert err <= max(10 * float(g['ref_fp32_grad_relerr']), 5e-3), err
    assert worst_norm <= 5e-2 and rel1(float(r0['total_norm']), float(g['total_norm64'])) < 5e-2


def _single_process_shard_sum(simq, spec, world):
    """What the ranks' all-reduce must produce, computed by ONE process: each shard's gradient through the ordinary (non-parallel)
    HIP step with the Huber sum scaled by 1/global_batch (lr = 0: the parameters stay put), summed in rank order."""
    from simq import dist as sdist
    from simq.learner import Transition, train_step
    cin, cout, gB, wseed, dseed, precision, tfrac, _ = spec
    dev = torch.device('cuda', 0)
    trs = _transitions(cin, cout, gB, dseed, tfrac)
    total, sums, bn0 = None, np.zeros(2), None
    for r in range(world):
        lo, hi = sdist.shard_bounds(gB, world, r)
        policy, target = _make_nets(simq, cin, cout, wseed, precision, dev)
        out = train_step(policy, target, Transition(*zip(*trs[lo:hi])), cases.GAMMA, hi - lo, 0.0, cases.MOMENTUM, 0.0, cases.CLIP,
                         use_double_dqn=True, global_batch=gB, sync=False)
        sums += np.asarray(out.tolist()[:2])
        g, _ = _unclipped(policy)
        total = g if total is None else total + g
        if r == 0:
            bn0 = policy.bn_buffers.cpu().numpy()
        del policy, target
    torch.cuda.empty_cache()
    return total, sums[0] / gB, sums[1] / gB, bn0


PROPERTY_CASES = [
    # configs[3] lifting_2_pushing_2: Cin 5, one net per robot group (Cout 2 and 1), 64 transitions per GPU and net, fp32
    ('configs3_lifting_c5o2_64perrank', (5, 2, 128, 61, 71, 'fp32', 0.1, 2), 2, 'gloo', False, 2e-4),
    ('configs3_pushing_c5o1_64perrank', (5, 1, 128, 62, 72, 'fp32', 0.1, 2), 2, 'gloo', False, 2e-4),
    # the same shard size through libsimq's RCCL communicator (one rank: the collectives run, the sum is the shard itself)
    ('configs3_lifting_c5o2_64_rccl_comm', (5, 2, 64, 61, 73, 'fp32', 0.1, 2), 1, 'nccl', True, 2e-4),
    # configs[4] lifting_4-large_empty: Cin 5, Cout 2, 128 transitions per GPU, bf16 operands
    ('configs4_c5o2_128perrank_bf16', (5, 2, 256, 63, 74, 'bf16', 0.1, 2), 2, 'gloo', False, 2e-3),
    ('configs4_c5o2_128_bf16_rccl_comm', (5, 2, 128, 63, 75, 'bf16', 0.1, 2), 1, 'nccl', True, 2e-3),
]


@pytest.mark.parametrize('name,spec,world,backend,use_comm,tol', PROPERTY_CASES, ids=[c[0] for c in PROPERTY_CASES])
def test_dp_step_full_size_properties(tmp_path, name, spec, world, backend, use_comm, tol):
    import simq
    ranks = _run_ranks(tmp_path, world, backend, use_comm, spec)
    r0 = ranks[0]
    for r in ranks[1:]:
        assert np.array_equal(r0['params'], r['params']) and np.array_equal(r0['momentum'], r['momentum'])
        assert np.array_equal(r0['grad'], r['grad']) and r['loss'] == r0['loss']
    assert np.isfinite(r0['params']).all() and np.isfinite(float(r0['loss_last']))
    want, loss, td, bn0 = _single_process_shard_sum(simq, spec, world)
    got = torch.as_tensor(r0['grad'])
    err = float((got - want).norm() / want.norm())
    print('%s: all-reduced gradient vs sum of single-process shard gradients: rel-L2 %.3g; loss %.6g vs %.6g' % (name, err, float(r0['loss']), loss))
    assert err <= tol, err
    assert abs(float(r0['loss']) - loss) <= 1e-5 * abs(loss) and abs(float(r0['td_error']) - td) <= 1e-5 * abs(td)
    assert np.abs(r0['bn'] - bn0).max() <= 1e-6 * np.abs(bn0).max()               # rank 0: statistics of ITS shard only
    # first SGD step identity on the all-reduced, clipped gradient: m = c*g + wd*p0 ; p1 = p0 - lr*m
    cin, cout, gB, wseed = spec[0], spec[1], spec[2], spec[3]
    p0 = _make_nets(simq, cin, cout, wseed, 'fp32', torch.device('cuda', 0))[0].flat_params.double().cpu()
    tn = float(r0['total_norm'])
    c = min(1.0, cases.CLIP / (tn + 1e-6))
    m = c * torch.as_tensor(r0['grad']) + cases.WEIGHT_DECAY * p0
    p1 = p0 - cases.LR * m
    assert float((torch.as_tensor(r0['params1']).double() - p1).norm() / p1.norm()) < 1e-6


SYNCBN_CASES = [('train_c4o2_b8', 2, 'gloo', False), ('train_c4o2_b8', 4, 'gloo', False), ('train_c5o1_b4', 2, 'gloo', False),
                ('train_c4o2_b8', 1, 'nccl', True)]


@pytest.mark.parametrize('name,world,backend,use_comm', SYNCBN_CASES, ids=['%s-w%d-%s' % (c[0], c[1], c[2]) for c in SYNCBN_CASES])
def test_dp_step_with_syncbn_equals_the_single_device_reference_step(tmp_path, golden_dir, name, world, backend, use_comm):
    """The SyncBN option: with the train-mode BatchNorm statistics reduced over the ranks -- forward sums, backward sums,
    the double-DQN forward over the non-final next states of ALL ranks, all-terminal shards contributing zeros -- an N-rank step IS
    the single-device step on the whole minibatch.  So it is held to the fixtures of the reference's own single-process train.train
    (tests/golden/train_*.npz): loss, td error, q_sa, TD targets at 1e-4, the all-reduced gradient against the fp64 summary.
    (train_c5o1_b4 on 4 ranks: one transition per rank, terminal ones included.)"""
    import simq
    _, cin, cout, gB, wseed, dseed = [c for c in cases.TRAIN_CASES if c[0] == name][0]
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    ranks = _run_ranks(tmp_path, world, backend, use_comm, (cin, cout, gB, wseed, dseed, 'fp32', 0.25, 1), sync_bn=True)
    r0 = ranks[0]
    for r in ranks[1:]:
        assert np.array_equal(r0['params'], r['params']) and np.array_equal(r0['grad'], r['grad'])
        # global statistics everywhere: every rank's running mean / var equal rank 0's -- including a rank whose shard is all
        # terminal, which normalises nothing in the double-DQN forward but commits the reduced statistics (simq_forward_sync_null)
        assert np.abs(r['bn'] - r0['bn']).max() <= 1e-6 * np.abs(r0['bn']).max()
    rel1 = lambda a, b: abs(a - b) / abs(b)
    assert rel1(float(r0['loss']), float(g['loss'][0])) < 1e-4 and rel1(float(r0['td_error']), float(g['td_error'][0])) < 1e-4
    q_sa, y = np.concatenate([r['q_sa'] for r in ranks]), np.concatenate([r['y'] for r in ranks])
    assert np.abs(q_sa - g['q_sa']).max() <= 1e-4 * np.abs(g['q_sa']).max()
    assert np.abs(y - g['y']).max() <= 1e-4 * np.abs(g['y']).max()
    err, worst_norm = _sampled_relerr(_reference_layout(simq, cin, cout, r0['grad']), g)
    print('%s on %d ranks with SyncBN: sampled-gradient rel-L2 error vs the single-device fp64 step %.3g (reference fp32: %.3g); '
          'total norm %.6g vs %.6g' % (name, world, err, float(g['ref_fp32_grad_relerr']), float(r0['total_norm']), float(g['total_norm64'])))
    assert err <= max(10 * float(g['ref_fp32_grad_relerr']), 5e-3), err
    assert rel1(float(r0['total_norm']), float(g['total_norm64'])) < 5e-2


def _literal_worker(rank, world, port, name, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import simq
        from simq.learner import Transition, train_step_dataparallel
        _, cin, cout, gB, w, wseed, dseed = [c for c in cases.DP_LITERAL_CASES if c[0] == name][0]
        batch = cases.make_batch(cin, cout, gB, dseed)
        policy, target = _make_nets(simq, cin, cout, wseed, 'fp32', dev)
        info = train_step_dataparallel(policy, target, Transition(*batch), cases.GAMMA, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, cases.CLIP,
                                       dist.group.WORLD)
        g, tn = _unclipped(policy)
        np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), grad=g.numpy(), total_norm=tn, loss=info['loss'], td_error=info['td_error'],
                 q_sa=policy._last['q_sa'].cpu().numpy(), y=policy._last['y'].cpu().numpy(), best=policy._last['best'].cpu().numpy(),
                 bn=policy.bn_buffers.cpu().numpy(), params=policy.flat_params.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('name', [c[0] for c in cases.DP_LITERAL_CASES])
def test_dataparallel_literal_step_against_reference_replicas(tmp_path, golden_dir, name):
    """simq.train_step_dataparallel: the double-DQN forward scattered the way nn.DataParallel scatters it -- torch.chunk pieces of the
    COMPACTED non-final next states, greedy actions exchanged between the ranks -- against tests/golden/dplit_*.npz (the reference's own
    modules replica by replica, oracle/gen_golden.py dp_literal).  Ranks share the GPU over gloo."""
    import simq
    _, cin, cout, gB, world, wseed, dseed = [c for c in cases.DP_LITERAL_CASES if c[0] == name][0]
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    ctx = mp.get_context('spawn')
    port = _free_port()
    procs = [ctx.Process(target=_literal_worker, args=(r, world, port, name, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
        assert not p.is_alive() and p.exitcode == 0, 'a data-parallel rank failed (exit code %r)' % p.exitcode
    ranks = [np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r)) for r in range(world)]
    r0 = ranks[0]
    for r in ranks:
        assert np.array_equal(r['best'], g['best'])                     # every rank holds the reference's greedy actions
        assert np.array_equal(r0['params'], r['params']) and np.array_equal(r0['grad'], r['grad'])
    rel1 = lambda a, b: abs(a - b) / abs(b)
    assert rel1(float(r0['loss']), float(g['loss'])) < 1e-4 and rel1(float(r0['td_error']), float(g['td_error'])) < 1e-4
    q_sa, y = np.concatenate([r['q_sa'] for r in ranks]), np.concatenate([r['y'] for r in ranks])
    assert np.abs(q_sa - g['q_sa']).max() <= 1e-4 * np.abs(g['q_sa']).max()
    assert np.abs(y - g['y']).max() <= 1e-4 * np.abs(g['y']).max()
    want, got = g['bn_buffers_after'].astype(np.float64), r0['bn'].astype(np.float64)     # replica 0: state chunk 0, compacted chunk 0
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    err, worst_norm = _sampled_relerr(_reference_layout(simq, cin, cout, r0['grad']), g)
    print('%s: sampled-gradient rel-L2 error %.3g (reference fp32 replicas: %.3g); slice sharding would give loss %.6g instead of %.6g'
          % (name, err, float(g['ref_fp32_grad_relerr']), float(g['slice_sharding_loss']), float(g['loss'])))
    assert err <= max(10 * float(g['ref_fp32_grad_relerr']), 5e-3), err
    assert rel1(float(r0['total_norm']), float(g['total_norm64'])) < 5e-2


needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two MI355X (RCCL refuses two ranks on one device)')


@needs_two_gpus
@pytest.mark.parametrize('name', ['dp_c5o2_b8_w2', 'dp_c5o1_b8_w2'])
def test_dp_step_over_rccl_between_two_gpus(tmp_path, golden_dir, name):
    """Two ranks on two GPUs over libsimq's RCCL communicator (use_comm: the fused data-parallel simq_train_step -- event-ordered
    bucket all-reduces on the communicator's stream, overlapped with backward phase 2) against the reference-replica fixtures."""
    test_dp_step_against_reference_replica_fixture(tmp_path, golden_dir, name, 'nccl', True)


@needs_two_gpus
def test_dp_syncbn_over_rccl_between_two_gpus(tmp_path, golden_dir):
    """SyncBN over simq_comm_reduce_f64 (44 small reductions per step inside the library) between two real ranks."""
    test_dp_step_with_syncbn_equals_the_single_device_reference_step(tmp_path, golden_dir, 'train_c4o2_b8', 2, 'nccl', True)


def _loss_timing_worker(port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        import simq
        from simq import dist as sdist
        from simq.learner import train_step
        cin, cout, B = 4, 2, 64
        policy, target = _make_nets(simq, cin, cout, 77, 'fp32', dev)
        comm = sdist.Comm(dist.group.WORLD)
        ring = simq.DeviceReplayBuffer(256, cin, device=dev)
        for t in _transitions(cin, cout, 256, 5, 0.1):
            ring.push(*t)
        import time
        busy, losses, sums = [], [], []
        for s in range(7):
            shard = ring.gather(ring.sample_indices(B), allow_all_final=True)
            info = train_step(policy, target, shard, cases.GAMMA, B, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, cases.CLIP,
                              use_double_dqn=True, global_batch=B, comm=comm)
            t0 = time.perf_counter()                     # the loss is on the host; how much of the step is the device still to run?
            torch.cuda.synchronize(dev)
            busy.append((time.perf_counter() - t0) * 1e3)
            losses.append(info['loss'])
            sums.append(float(torch.nn.functional.smooth_l1_loss(policy._last['q_sa'], policy._last['y'], reduction='sum')) / B)
        comm.close()
        np.savez(os.path.join(out_dir, 'loss_timing.npz'), busy=np.array(busy), loss=np.array(losses), loss_from_rows=np.array(sums))
    finally:
        dist.destroy_process_group()


def test_dp_step_hands_the_loss_to_the_host_before_its_backward_pass_ends(tmp_path):
    """Round 6: in the data-parallel form of simq_train_step the four loss sums are all-reduced right behind the TD / Huber launch and copied
    to the host from the communicator's stream -- not behind the second gradient bucket.  A host that reads the loss every step
    (train.py:137-139) therefore gets it while the backward pass of the same step still runs and enqueues the next step beside it (with the
    loss behind bucket 2 the 1-rank form measured 6.5 % slower than the plain step: profiles/r06_ab_early_target_delay_dp.txt).  1-rank RCCL
    communicator, 64 transitions: when train_step returns, the device still has more than 1.5 ms of the step to run (the backward pass of 64
    transitions takes ~5 ms; behind bucket 2 only clip + SGD + the weight-cache refresh, ~0.2 ms, were left) in at least 5 of the 6
    steady-state steps (a descheduled host thread may miss one), and the loss it returned is the mean Huber term of the rows the step left."""
    ctx = mp.get_context('spawn')
    p = ctx.Process(target=_loss_timing_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    p.join(600)
    if p.is_alive():
        p.kill()
        pytest.fail('the 1-rank data-parallel worker did not finish (hang)')
    assert p.exitcode == 0
    r = np.load(os.path.join(str(tmp_path), 'loss_timing.npz'))
    print('device time left when the loss reached the host, ms per step:', np.round(r['busy'], 2))
    assert int((r['busy'][1:] > 1.5).sum()) >= 5, r['busy']
    assert np.allclose(r['loss'], r['loss_from_rows'], rtol=1e-5, atol=1e-7), (r['loss'], r['loss_from_rows'])


def _bench_line(argv, timeout=900):
    """bench.py started BARE (no launcher, no WORLD_SIZE in the environment) -- the way the driver starts `--gpus 1` -- and its one
    JSON line."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, 'bench.py %s exited %d\n%s\n%s' % (' '.join(argv), r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks_from_a_bare_process():
    """`python bench.py --gpus 2` with no launcher around it starts its own two ranks (torch.distributed.run on 127.0.0.1; here they
    share the one GPU over gloo), rank 0 prints the line: BASELINE configs[1] sharded over the ranks as the headline, the
    weak-scaling leg beside it, a per-rank roofline."""
    line = _bench_line(['--gpus', '2', '--backend', 'gloo', '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline', '--replay', '256'])
    assert line['n_gpus'] == 2 and line['steps'] == 2 and line['unit'] == 'transitions/s' and line['value'] > 0
    cfg = line['config']
    assert cfg['workload_key'] == 'configs1' and cfg['global_batch'] == 32 and cfg['per_gpu_batch'] == 16 and cfg['parallelism'] == 'dp2'
    assert line['scaling'] == 'strong' and line['dtype'] == 'f32'
    assert 'torch.distributed (gloo)' in cfg['gradient_transport']
    assert np.isfinite(cfg['last_loss']) and line['value_fwd_bwd_only'] > 0
    assert abs(line['value'] - 32 * 2 / (line['ms_per_step'] * 2e-3)) <= 1e-3 * line['value']
    roof = line['roofline']
    assert roof['frac'] > 0 and [r['rank'] for r in roof['per_rank']] == [0, 1] and all(r['frac'] > 0 for r in roof['per_rank'])
    weak = line['weak32']
    assert weak['scaling'] == 'weak' and weak['full_step_transitions_per_s'] > 0 and '64' in weak['workload']


def test_bench_maps_gpu_counts_to_the_baseline_configs():
    """--workload at one GPU: configs[3]'s two heterogeneous nets (one loop pass of train.py:255-257 = 2 x 256 transitions) and
    configs[4]'s net in bf16, at reduced step counts; the line names what ran."""
    line = _bench_line(['--workload', 'configs3', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-roofline', '--no-m1',
                        '--batch', '16', '--replay', '128'])
    cfg = line['config']
    assert cfg['workload_key'] == 'configs3' and cfg['nets'] == 2 and cfg['transitions_per_step'] == 32 and line['dtype'] == 'f32'
    assert 'Cin=5->Cout=2 + Cin=5->Cout=1' in cfg['workload'] and np.isfinite(cfg['last_loss'])
    line = _bench_line(['--workload', 'configs4', '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline', '--no-m1', '--batch', '128',
                        '--replay', '256'])
    assert line['config']['workload_key'] == 'configs4' and line['dtype'].startswith('bf16') and line['roofline']['peak'] == 2500.0
    assert line['roofline']['traffic_source'] is None or line['roofline']['traffic_source'].startswith('profiles/')


def test_bench_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) prints the headline line and nothing beside it; --dump-outputs writes what the last timed step left a
    caller of train() holding, and two runs with the same (default) arguments write the same arrays bit for bit: the headline workload
    runs deterministic plans, and the other legs' plans are not part of a plain run."""
    argv = ['--steps', '20', '--warmup', '3']
    dumps = []
    for run in range(2):
        d = tmp_path / ('run%d' % run)
        line = _bench_line(argv + ['--dump-outputs', str(d)])
        assert line['steps'] == 20 and line['unit'] == 'transitions/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
        assert line['config']['workload_key'] == 'configs1' and line['value'] > 0
        assert abs(line['value'] - 32 * 20 / (line['ms_per_step'] * 20e-3)) <= 1e-3 * line['value']
        assert line['config']['deterministic_plans'] is True
        for key in ('roofline', 'cpu_baseline', 'sustained', 'value_fwd_bwd_only'):
            assert line[key] is None, key
        assert 'bf16_configs2' not in line and 'fp32_mfma_configs1' not in line
        files = sorted(os.listdir(str(d)))
        assert files == ['loss.npy', 'momentum.npy', 'policy_state.npy', 'td_error.npy'], files
        arrays = {f[:-4]: np.load(str(d / f)) for f in files}
        assert sum(os.path.getsize(str(d / f)) for f in files) <= 64 << 20
        assert arrays['loss'].dtype == np.float64 and arrays['loss'][0] == line['config']['last_loss']
        assert arrays['td_error'][0] == line['config']['last_td_error']
        for k in ('policy_state', 'momentum'):
            assert arrays[k].dtype == np.float32 and arrays[k].ndim == 1 and arrays[k].size > 10 ** 6 and np.isfinite(arrays[k]).all(), k
        assert np.abs(arrays['momentum']).max() > 0
        dumps.append(arrays)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k

#!/usr/bin/env python3
"""GPU box.  Two probes of the F(4x4,3x3) convolution's transform kernels on the step's own shapes:

  wino4f_probe.py [B ...]          under `rocprofv3 --kernel-trace`: the whole operator (input transform, 36 batched GEMMs, output transform
                                   with BatchNorm statistics), so that the transform kernels can be read per (kernel, grid) from the trace
                                   (tools/wino4f_trace.py; recipe `w4f`)
  wino4f_probe.py forms MANIFEST [B ...]   likewise under a kernel trace: the OUTPUT transform alone (simq_wino4f_output) in every form the step launches -- plain,
                                   eval (folded BatchNorm + residual + ReLU), batch statistics, dgrad with the fused BatchNorm-backward sums
                                   of one and of two BatchNorms -- at 128 / 256 / 512 channels: one line per form and shape with the
                                   one-pixel-at-a-time kernel (form 0, the parent's), the two-phase kernel (form 1) and the two-phase kernel's
                                   timing ablations (ablation build: fold without atomics; no sums; no epilogue loads), beside the bare
                                   transform (plain form, no bias) scaled by the bytes the form moves.  All variants of a line run in
                                   interleaved rounds in one process, each launch alone on the device, over buffer sets that rotate through
                                   more than the 256 MB of last-level cache; MANIFEST (written at the end) names every launch in order, and
                                   `tools/wino4f_trace.py forms results.db MANIFEST` prints the table (recipe `w4f_forms`).
"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd')]
os.environ.setdefault('SIMQ_LIBRARY', os.path.join(ROOT, 'spatial-intention-maps_amd', 'simq', 'libsimq_ablate.so'))
import torch  # noqa: E402
from simq import _lib as L  # noqa: E402
H = 24


def operator_probe(batches):
    st = L.stream_ptr()
    for B in batches:
        for cin, cout in [(512, 512), (256, 512), (512, 256), (256, 256), (128, 256), (256, 128), (128, 128)]:
            x = torch.randn(B, H, H, cin, device='cuda')
            w = torch.randn(cout, 3, 3, cin, device='cuda') * (cin * 9) ** -0.5
            b = torch.randn(cout, device='cuda')
            y = torch.empty(B, H, H, cout, device='cuda')
            stats = torch.zeros(2 * cout, dtype=torch.float64, device='cuda')
            T = B * (H // 2) ** 2
            scratch = torch.empty(36 * cout * cin + 16 * T * (cin + cout), device='cuda')
            for _ in range(12):
                L.lib.call('simq_conv2d_fwd_winograd4', L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, H, H, cin, cout, L.ptr(stats), L.ptr(scratch), st, None)
            torch.cuda.synchronize()
            ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), padding=1).permute(0, 2, 3, 1)
            err = float((y - ref).abs().max() / ref.abs().max())
            s_ref = torch.cat([ref.sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))]) * 12
            s_mag = torch.cat([ref.abs().sum((0, 1, 2)), (ref * ref).sum((0, 1, 2))]) * 12      # a sum's error against the sum of magnitudes
            serr = float(((stats - s_ref).abs() / s_mag).max())
            print('B=%d %d->%d  max err vs fp64 %.2e  statistics %.2e' % (B, cin, cout, err, serr))
            assert err < 2e-5 and serr < 1e-5, (err, serr)


# form name -> (activation-shaped tensors read beside Mt, per-channel vectors, fp64 sums, relu)
FORMS = {
    'bare': ((), (), (), False),
    'plain': ((), ('bias',), (), False),
    'eval': (('addend',), ('bias', 'scale', 'shift'), (), True),
    'stats': ((), ('bias',), ('stats',), False),
    'dgrad1 recomputed mask': (('bnr_y1',), ('bnr_mscale', 'bnr_mshift', 'bnr_mean1', 'bnr_invstd1'), ('bnr_red1',), False),
    'dgrad1 mask tensor': (('bnr_y1', 'bnr_mask'), ('bnr_mean1', 'bnr_invstd1'), ('bnr_red1',), False),
    'dgrad1 mask + addend': (('bnr_y1', 'bnr_mask', 'addend'), ('bnr_mean1', 'bnr_invstd1'), ('bnr_red1',), False),
    'dgrad2 mask tensor': (('bnr_y1', 'bnr_mask', 'bnr_y2'), ('bnr_mean1', 'bnr_invstd1', 'bnr_mean2', 'bnr_invstd2'), ('bnr_red1', 'bnr_red2'), False),
}
ROUNDS = 7


def forms_probe(batches, manifest_path):
    """Launches only (run it under `rocprofv3 --kernel-trace`); the manifest names every launch in order for tools/wino4f_trace.py forms."""
    ablate = L.lib.build_flags != 0
    variants = [('form0', 0), ('form1', 1)] + ([('no atomics', 1 + 16), ('no sums', 1 + 32), ('no epi loads', 1 + 64)] if ablate else [])
    manifest = []
    for B in batches:
        for C in (128, 256, 512):
            T4 = B * (H // 4) ** 2
            SETS = min(24, max(4, int(600e6 / (B * H * H * C * 4 * 3.25)) + 1))      # the smallest form's sets rotate through > 600 MB
            mt = [torch.randn(36, T4, C, device='cuda') for _ in range(SETS)]
            ys = [torch.empty(B, H, H, C, device='cuda') for _ in range(SETS)]
            for name, (acts, vecs, sums, relu) in FORMS.items():
                tens = {n: [torch.randn(B, H, H, C, device='cuda') for _ in range(SETS)] for n in acts}
                tens.update({n: [torch.rand(C, device='cuda') + 0.5 for _ in range(SETS)] for n in vecs})
                tens.update({n: [torch.zeros(2 * C, dtype=torch.float64, device='cuda') for _ in range(SETS)] for n in sums})
                vs = [v for v in variants if v[1] < 2 or (v[0] == 'no epi loads' and acts) or (v[0] != 'no epi loads' and sums)]
                mb = B * H * H * C * 4 * (2.25 + 1 + len(acts)) / 1e6      # Mt (36 / 16 of y) + y + the activation-shaped tensors read
                for rnd in range(-1, ROUNDS):            # round -1: warm-up (code objects, clocks), not reported
                    for vn, f in vs:
                        for s in range(SETS):
                            L.wino4f_output(mt[s], ys[s], form=f, relu=relu, **{n: t[s] for n, t in tens.items()})
                            manifest.append([B, C, name, mb, vn, rnd])
                torch.cuda.synchronize()
                del tens
    with open(manifest_path, 'w') as f:
        json.dump(manifest, f)
    print('%d launches, manifest %s' % (len(manifest), manifest_path))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == 'forms':
        forms_probe([int(a) for a in args[2:]] or [32, 29], args[1])
    else:
        operator_probe([int(a) for a in args] or [32, 29])

#!/usr/bin/env python3
"""GPU: round-off of the two forms of the batched transform-domain GEMM against fp64 -- simq_gemm_f32_batched with gemm_split = 0
(v_mfma_f32_16x16x4_f32 on the fp32 operands) and 1 (bf16 matrix cores, exact three-way operand split, six partial products) -- on
operands shaped like the Winograd planes (random normal; a wide-dynamic-range case; all-positive operands; and the `adversarial` class:
all positive with mantissa 0x00FFFF and exponents in [-2, 2], for which the three piece products the split form drops reach 0.97 2^-21
of every product, all of one sign -- tests/split3_oracle.py).  Prints max / rms error relative to the rms of the exact result, the ratio
split / fp32-MFMA, and the mean signed error relative to the mean magnitude of the result in units of 2^-21 (the bias: about -0.97 on the adversarial
class for the split form, 0 for fp32 MFMA).   usage: tools/gemm_split_accuracy.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd')]
import torch
from simq import _lib as L
st = L.stream_ptr()
torch.manual_seed(0)
for name, M, N, K, P, kind in (('normal', 1152, 512, 512, 36, 0), ('normal', 1044, 256, 128, 36, 0), ('normal', 512, 512, 1152, 36, 0),
                               ('normal', 4176, 128, 128, 16, 0), ('wide range', 1152, 256, 256, 8, 1), ('one-signed', 1152, 256, 256, 8, 2),
                               ('adversarial', 1152, 256, 256, 8, 3), ('adversarial', 128, 128, 512, 2, 3)):
    x = torch.randn(P, M, K, device='cuda'); w = torch.randn(P, N, K, device='cuda')
    if kind == 1:
        x = x * torch.exp2(torch.randint(-20, 20, x.shape, device='cuda').float()); w = w * torch.exp2(torch.randint(-20, 20, w.shape, device='cuda').float())
    if kind == 2:
        x, w = x.abs(), w.abs()
    if kind == 3:
        adv = lambda t: ((torch.randint(125, 130, t.shape, device='cuda', dtype=torch.int32) << 23) | 0x00FFFF).view(torch.float32)
        x, w = adv(x), adv(w)
    ref = torch.bmm(x.double(), w.double().transpose(1, 2))
    scale = float(ref.pow(2).mean().sqrt())
    out = {}
    for split in (0, 1):
        y = torch.full((P, M, N), float('nan'), device='cuda')
        L.lib.call('simq_gemm_f32_batched', L.ptr(x), L.ptr(w), L.ptr(y), M, N, K, P, st, opts=L.launch_opts(gemm_split=split))
        torch.cuda.synchronize()
        d = (y.double() - ref)
        out[split] = (float(d.abs().max()) / scale, float(d.pow(2).mean().sqrt()) / scale, float(d.mean() / ref.abs().mean()) * 2.0 ** 21)
    tm = torch.bmm(x, w.transpose(1, 2)).double() - ref
    print('%-11s M=%5d N=%4d K=%5d x%2d   fp32 MFMA: max %.3e rms %.3e   split3: max %.3e rms %.3e   (split / fp32: max %.2f rms %.2f)   mean error / mean |result| [2^-21]: fp32 %+.3f split3 %+.3f   torch.bmm fp32 rms %.3e' % (
        name, M, N, K, P, out[0][0], out[0][1], out[1][0], out[1][1], out[1][0] / out[0][0], out[1][1] / out[0][1], out[0][2], out[1][2], float(tm.pow(2).mean().sqrt()) / scale), flush=True)

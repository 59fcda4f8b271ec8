"""GPU: the F(4x4,3x3) output transform on its own (simq_wino4f_output).  Form 1 -- the two-phase kernel the plans launch: a tile's
epilogue loads issued back to back, then its arithmetic, then its stores -- against form 0, the one-pixel-at-a-time kernel it replaced,
kept verbatim as the oracle.  The two perform the same operations in the same order on every value and every accumulator, so y is
compared bit for bit on any data, and the fp64 sums bit for bit on data for which they are exact:

  every input is a multiple of 2^-4 (2^-2 for the per-channel vectors) of magnitude <= 4.  A^T m A has coefficients down to 1/8 per side,
  so a transformed value is a multiple of 2^-10 below 2^9: exact in fp32.  Behind it the epilogue multiplies and adds grid values; fp32
  rounding only drops low bits, so every partial sum a thread hands to the fp64 stage is a multiple of 2^-30 below 2^22 -- 52 bits:
  the fp64 additions are exact in any order, whichever block's atomic arrives first.  (Asserted as a precondition: form 0 twice.)

Shapes: the smallest that take each loop of the kernel 0, 1 and several times (the table in the docstring of SHAPES)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# C, B, H = W    T4 tiles   what it exercises
SHAPES = [
    (64, 1, 4),      # 1      no channel slicing (16 quads = one slice); fewer tiles than one block holds
    (128, 3, 12),    # 27     two slices; ragged last block (16 tiles per block)
    (512, 2, 24),    # 72     eight slices
    (512, 58, 24),   # 2088   more than 128 x 16 tiles: the blocks of the forms that leave sums take two grid-stride trips
]
KINDS = ['plain', 'eval', 'eval_inplace', 'stats', 'dgrad_mask', 'dgrad_recomputed', 'dgrad_two_bn', 'dgrad_mask16_addend']


@pytest.fixture(scope='module')
def L():
    from simq import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return _lib


def grid(gen, shape, step=16, maxabs=4):
    """multiples of 1 / step in [-maxabs, maxabs]"""
    return torch.randint(-maxabs * step, maxabs * step + 1, shape, generator=gen, device='cuda').float() / step


def make_case(kind, C, B, H, randn=False, seed=0):
    """(mt, epilogue tensors by field name, relu, names of the fp64 sums, initial y or None)"""
    gen = torch.Generator(device='cuda').manual_seed(1000 * seed + 7 * C + 3 * B + H)
    T4 = B * (H // 4) ** 2
    if randn:
        act = lambda: torch.randn(B, H, H, C, generator=gen, device='cuda')
        vec = lambda: torch.randn(C, generator=gen, device='cuda')
        mt = torch.randn(36, T4, C, generator=gen, device='cuda')
    else:
        act = lambda: grid(gen, (B, H, H, C))
        vec = lambda: grid(gen, (C,), step=4, maxabs=2)
        mt = grid(gen, (36, T4, C))
    zsum = lambda: torch.zeros(2 * C, dtype=torch.float64, device='cuda')
    t, relu, sums, y0 = {'bias': vec()}, False, [], None
    if kind == 'plain':
        pass
    elif kind in ('eval', 'eval_inplace'):
        t.update(scale=vec(), shift=vec(), addend=act())
        relu = True
        if kind == 'eval_inplace':
            y0 = t['addend']          # the residual is added in place: addend aliases y
    elif kind == 'stats':
        t.update(stats=zsum())
        sums = ['stats']
    else:
        t.update(bnr_y1=act(), bnr_mean1=vec(), bnr_invstd1=vec().abs() + 0.25, bnr_red1=zsum())
        sums = ['bnr_red1']
        if kind == 'dgrad_mask':
            t.update(bnr_mask=act())
        elif kind == 'dgrad_recomputed':
            t.update(bnr_mscale=vec(), bnr_mshift=vec())
        elif kind == 'dgrad_two_bn':
            t.update(bnr_mask=act(), addend=act(), bnr_y2=act(), bnr_mean2=vec(), bnr_invstd2=vec().abs() + 0.25, bnr_red2=zsum())
            sums = ['bnr_red1', 'bnr_red2']
        elif kind == 'dgrad_mask16_addend':
            t.update(bnr_mask16=act().bfloat16().view(torch.int16), addend=act())
        else:
            raise AssertionError(kind)
    return mt, t, relu, sums, y0


def run(L, form, B, H, C, mt, t, relu, sums, y0):
    y = torch.full((B, H, H, C), float('nan'), device='cuda') if y0 is None else y0.clone()
    t = dict(t)
    for s in sums:
        t[s] = torch.zeros_like(t[s])
    if y0 is not None:
        t['addend'] = y
    L.wino4f_output(mt, y, form=form, relu=relu, **t)
    torch.cuda.synchronize()
    return y, [t[s] for s in sums]


@pytest.mark.parametrize('C,B,H', SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('kind', KINDS)
def test_two_phase_kernel_equals_the_one_pixel_kernel_bit_for_bit(L, kind, C, B, H):
    case = make_case(kind, C, B, H)
    y0, s0 = run(L, 0, B, H, C, *case)
    y0b, s0b = run(L, 0, B, H, C, *case)
    assert torch.equal(y0, y0b) and all(torch.equal(a, b) for a, b in zip(s0, s0b)), 'precondition: the oracle is not reproducible on grid data'
    assert not torch.isnan(y0).any() and float(y0.abs().max()) > 0
    for s in s0:
        assert float(s.abs().max()) > 0          # the sums were written (not all-zero masks)
    y1, s1 = run(L, 1, B, H, C, *case)
    assert torch.equal(y1, y0), 'y differs: %d of %d values' % (int((y1 != y0).sum()), y0.numel())
    assert len(s1) == len(s0)
    for a, b in zip(s1, s0):
        assert torch.equal(a, b), 'sums differ: max |d| %.3e' % float((a - b).abs().max())


@pytest.mark.parametrize('C,B,H', [(128, 3, 12), (512, 2, 24)], ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['eval', 'stats', 'dgrad_recomputed', 'dgrad_two_bn'])
def test_two_phase_kernel_on_random_data(L, kind, C, B, H):
    """randn inputs: y bit for bit; the fp64 sums to 1e-12 (fp32 partials added in fp64 in the order the blocks arrive: at most 128
    additions per sum, each within 2^-53 of the running magnitude -- orders of magnitude inside 1e-12 of the largest sum)."""
    case = make_case(kind, C, B, H, randn=True, seed=1)
    y0, s0 = run(L, 0, B, H, C, *case)
    y1, s1 = run(L, 1, B, H, C, *case)
    assert torch.equal(y1, y0)
    for a, b in zip(s1, s0):
        d, tol = (a - b).abs(), 1e-12 * (b.abs() + float(b.abs().max()))
        print('%s C=%d: sums max |d| %.3e, largest |sum| %.3e' % (kind, C, float(d.max()), float(b.abs().max())))
        assert bool((d <= tol).all()), float((d / tol).max())


def test_bad_arguments_are_refused(L):
    mt, y = torch.zeros(36, 1, 64, device='cuda'), torch.zeros(1, 4, 4, 64, device='cuda')
    with pytest.raises(L.SimqError):
        L.wino4f_output(mt, y, form=7)
    with pytest.raises(L.SimqError):                     # bnr_red1 without the tensors it is formed from
        L.wino4f_output(mt, y, bnr_red1=torch.zeros(128, dtype=torch.float64, device='cuda'))
    with pytest.raises(L.SimqError):                     # a map that is no multiple of the 4x4 tile
        L.wino4f_output(mt, torch.zeros(1, 6, 6, 64, device='cuda'))
    with pytest.raises(L.SimqError):
        L.wino4f_output(mt, y, nonsense=None)

"""numpy model of the split-bf16 GEMM (csrc/gemm_split3.hip): which terms of  y = x w^T  the kernel keeps and which it drops.

The kernel cuts every fp32 operand into three bf16 pieces BY TRUNCATION,
      a = a0 + a1 + a2,     a0 = a & 0xffff0000,  a1 = (a - a0) & 0xffff0000,  a2 = upper 16 bits of (a - a0 - a1)
and accumulates six of the nine piece products,  kept = sum_{i+j<=2} a_i b_j,  in the fp32 accumulators of the matrix core; the three with
i + j >= 3 (a1 b2 + a2 b1 + a2 b2 = `dropped`) are never formed.  What follows from the truncation, for every NORMAL fp32 value:
      |a1| < 2^-7 |a|,  |a2| < 2^-15 |a|,  every piece carries a's sign or is zero
so per product  |dropped| < (2^-22 + 2^-22 + 2^-30) |a b|  and the dropped term has the product's sign: a one-signed bias towards zero of
up to 2^-21 (about 4 fp32 ulp of the product), not zero-mean round-off.

Domain.  Every subtraction is exact and every piece has zero low 16 bits while the lowest set bit of the operand is at or above 2^-133
(the 16th bit of the subnormal grid): every fp32 value of magnitude >= 2^-110.  Below that the bits under 2^-133 are lost (`split3` models
the truncation of the third piece the kernel's byte permute performs).  What the MATRIX CORE does with a piece below 2^-126 (a subnormal
bf16 value) is not modelled here: the bit-exact statements hold for pieces >= 2^-126, tests/test_gpu_split3.py reports what happens below.

`exact_operands` builds operands for which every kept product and every partial sum of them, in any order, is exactly representable in
fp32: for these the kernel's output is determined bit for bit (= `kept`), and differs from the correctly rounded full product.
"""
import numpy as np

MASK = np.uint32(0xffff0000)
EXACT_SUPPORT = 16                       # nonzero k positions per plane of exact_operands
EXACT_GRANULE = 2.0 ** -18               # every kept product of exact_operands is a multiple of this


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def split3(v):
    """(p0, p1, p2) fp32 arrays: the three pieces gemm_split3.hip's split3() hands to the matrix core for fp32 `v`, bit for bit (mask,
    exact fp32 subtract, mask, exact fp32 subtract, upper 16 bits)."""
    v = _f32(v)
    with np.errstate(invalid='ignore'):                                  # Inf - Inf = NaN, as on the device
        p0 = (v.view(np.uint32) & MASK).view(np.float32)
        r1 = v - p0
        p1 = (r1.view(np.uint32) & MASK).view(np.float32)
        r2 = r1 - p1
        p2 = (r2.view(np.uint32) & MASK).view(np.float32)
    return p0, p1, p2


def _mm(a, b):
    return np.matmul(a.astype(np.float64), np.swapaxes(b.astype(np.float64), -1, -2))


def kept(x, w):
    """fp64 [..., M, N]: the six piece products with i + j <= 2 of x [..., M, K] and w [..., N, K], summed over K."""
    a0, a1, a2 = (p.astype(np.float64) for p in split3(x))
    b0, b1, b2 = (p.astype(np.float64) for p in split3(w))
    return _mm(a0, b0 + b1 + b2) + _mm(a1, b0 + b1) + _mm(a2, b0)       # (sums of pieces are exact in fp64: 24 bits)


def dropped(x, w):
    """fp64 [..., M, N]: the three piece products with i + j >= 3."""
    _, a1, a2 = (p.astype(np.float64) for p in split3(x))
    _, b1, b2 = (p.astype(np.float64) for p in split3(w))
    return _mm(a1, b2) + _mm(a2, b1 + b2)


def full(x, w):
    """fp64 [..., M, N]: x w^T."""
    return _mm(_f32(x), _f32(w))


def abs_full(x, w):
    """fp64 [..., M, N]: sum_k |x||w|, the scale of the per-product bounds."""
    return _mm(np.abs(_f32(x)), np.abs(_f32(w)))


def exact_support(rng, planes, K, n=EXACT_SUPPORT):
    """int [planes, n]: n distinct k positions per plane, at least one in every 16-wide K-step where the K-steps are at most n."""
    steps = K // 16
    assert K % 16 == 0 and n <= K
    out = np.empty((planes, n), dtype=np.int64)
    for g in range(planes):
        if steps <= n:
            first = np.arange(steps) * 16 + rng.integers(0, 16, steps)
        else:
            first = np.empty(0, dtype=np.int64)
        rest = np.setdiff1d(np.arange(K), first)
        out[g] = np.sort(np.concatenate([first, rng.choice(rest, n - len(first), replace=False)]))
    return out


def exact_pieces(rng, shape):
    """(v0, v1, v2, sign) integer arrays: a value is sign * (v0 2^-1 + v1 2^-9 + v2 2^-17), v0, v1 in {2, 3}, v2 in {1, 2, 3}."""
    return rng.integers(2, 4, shape), rng.integers(2, 4, shape), rng.integers(1, 4, shape), rng.choice(np.array([-1.0, 1.0]), shape)


def exact_operands(rng, rows, K, support, return_pieces=False):
    """fp32 [planes, rows, K], zero except at the plane's `support` (exact_support) positions, where it holds
    +-(v0 2^-1 + v1 2^-9 + v2 2^-17).  split3 returns exactly those three terms, all nonzero; a kept product of two such operands is a
    multiple of 2^-18 below 2.27, so with 16 positions  sum |kept| < 36.3 < 2^-18 2^24 = 64:  every partial sum, in any order, is an
    integer multiple of 2^-18 below 2^24 of them -- exact in fp32.  The dropped products are multiples of 2^-34 below 2^-22: they move
    the correctly rounded full product away from `kept` in most outputs."""
    planes, n = support.shape
    v0, v1, v2, sign = exact_pieces(rng, (planes, rows, n))
    pieces = [sign * v0 * 2.0 ** -1, sign * v1 * 2.0 ** -9, sign * v2 * 2.0 ** -17]
    out = np.zeros((planes, rows, K), dtype=np.float32)
    idx = np.broadcast_to(support[:, None, :], (planes, rows, n))
    np.put_along_axis(out, idx, (pieces[0] + pieces[1] + pieces[2]).astype(np.float32), axis=2)
    if not return_pieces:
        return out
    planes_of = []
    for p in pieces:
        full_p = np.zeros((planes, rows, K), dtype=np.float32)
        np.put_along_axis(full_p, idx, p.astype(np.float32), axis=2)
        planes_of.append(full_p)
    return out, planes_of


def adversarial_operands(rng, rows, K, planes=1):
    """fp32 [planes, rows, K], all positive, mantissa 0x00FFFF (1 + 2^-7 - 2^-23: seven zero bits, then sixteen ones), exponents in
    [-2, 2]: the first piece is a power of two and the other two are as large as truncation lets them be -- a1 = (1 - 2^-8) 2^-7 a0,
    a2 = (1 - 2^-8) 2^-15 a0 -- so dropped / full is about 0.97 2^-21 in every product, all of one sign."""
    e = rng.integers(-2, 3, (planes, rows, K)).astype(np.uint32)
    return (((np.uint32(127) + e) << np.uint32(23)) | np.uint32(0x00FFFF)).view(np.float32)


def clamped_randn(rng, shape):
    """randn with magnitudes clamped into [2^-4, 2^4] (sign kept): every value's lowest bit is at or above 2^-27."""
    v = rng.standard_normal(shape)
    return (np.sign(v) * np.clip(np.abs(v), 2.0 ** -4, 2.0 ** 4)).astype(np.float32)


def low_bit(v):
    """fp64 array: the value of the lowest set bit of each nonzero finite fp32/fp64 element (inf where the element is zero)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    m, e = np.frexp(v)                                                   # v = m 2^e, m in [0.5, 1): a 53-bit integer times 2^(e - 53)
    i = np.round(np.ldexp(m, 53)).astype(np.int64)
    low = i & -i
    with np.errstate(over='ignore'):
        return np.where(v == 0, np.inf, np.ldexp(low.astype(np.float64), e - 53))


# the shapes tests/test_gpu_split3.py runs; tests/test_split3_model_cpu.py checks the operand constructions on the very same ones
EXACT_CASES = [
    # M, N, K, P
    (70, 128, 16, 1),            # one K-step: the tail only
    (64, 128, 32, 2),            # one loop trip, no tail
    (70, 128, 80, 3),            # ragged rows, loop + tail
    (200, 256, 64, 9),           # two row tiles, the wide tile, nine planes (the launcher walks them in launch order: four / two tiles do
                                 # not divide over the eight XCDs that would share the ninth plane)
    (200, 256, 64, 12),          # ... twelve planes: eight whole planes per XCD, the last four shared by two XCDs each
    (130, 256, 256, 8),          # whole planes per XCD
]
ADVERSARIAL_CASES = [(128, 128, 512, 2), (70, 256, 512, 3)]
SCALING_CASE = (130, 256, 80, 8)
SCALINGS = [(-40, -30), (60, -60), (-90, 90), (50, 50)]
TINY_SCALING = (-120, 100)


def exact_case(M, N, K, P, with_pieces=False):
    """The seeded exact operands of one EXACT_CASES entry: (x [P, M, K], w [P, N, K]) -- one support per plane, shared by both."""
    rng = np.random.default_rng(1000 + M + N + K + P)
    support = exact_support(rng, P, K)
    return exact_operands(rng, M, K, support, with_pieces), exact_operands(rng, N, K, support, with_pieces)


def adversarial_case(M, N, K, P):
    rng = np.random.default_rng(2000 + M + N + K + P)
    return adversarial_operands(rng, M, K, P), adversarial_operands(rng, N, K, P)


def scaling_case():
    M, N, K, P = SCALING_CASE
    rng = np.random.default_rng(3000 + M + N + K + P)
    return clamped_randn(rng, (P, M, K)), clamped_randn(rng, (P, N, K))

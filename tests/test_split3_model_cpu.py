"""CPU: the numpy model of the split-bf16 GEMM (tests/split3_oracle.py) against what it claims -- the decomposition, the bound on the
dropped piece products and their sign, and the operand constructions tests/test_gpu_split3.py relies on (so that no GPU test can pass
vacuously).  Every bound here is derived from the truncating split (see the oracle's docstring), none is taken from a kernel's output."""
import numpy as np
import pytest

import split3_oracle as S


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def _edge_values():
    exps = np.arange(1, 255, dtype=np.uint32)                            # every normal exponent field
    vals = [_bits((exps << np.uint32(23)) | np.uint32(m)) for m in (0x000000, 0x7FFFFF, 0x00FFFF)]
    vals.append(np.array([0.0, -0.0, np.finfo(np.float32).tiny, np.finfo(np.float32).max], dtype=np.float32))
    v = np.concatenate(vals)
    return np.concatenate([v, -v])


def _random_patterns(n, seed):
    rng = np.random.default_rng(seed)
    v = _bits(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    return v[np.isfinite(v)]


def test_the_decomposition_is_exact_truncating_and_sign_preserving():
    v = np.concatenate([_random_patterns(2_000_000, 1), _edge_values()])
    p0, p1, p2 = S.split3(v)
    v64, s = v.astype(np.float64), p0.astype(np.float64) + p1.astype(np.float64) + p2.astype(np.float64)
    for p in (p0, p1, p2):
        assert not (p.view(np.uint32) & np.uint32(0xffff)).any()                        # bf16 values, all of them
        assert ((np.sign(p) == np.sign(v)) | (p == 0)).all()                             # the sign of v, or zero
    # lowest bit at or above 2^-133 (every magnitude >= 2^-110): nothing is lost; below, only the bits under 2^-133 are
    whole = (np.abs(v64) >= 2.0 ** -110) | (v64 == 0)
    assert whole.sum() > 0.8 * v.size
    assert (s[whole] == v64[whole]).all()
    assert (np.abs(s - v64)[~whole] < 2.0 ** -133).all()
    normal = np.abs(v64) >= 2.0 ** -126
    a = np.abs(v64[normal])
    assert (np.abs(p1.astype(np.float64))[normal] < 2.0 ** -7 * a).all()
    assert (np.abs(p2.astype(np.float64))[normal] < 2.0 ** -15 * a).all()
    # ... and the bounds are nearly reached (truncation, not rounding: a round-to-nearest split would stay below half of these)
    assert (np.abs(p1.astype(np.float64))[normal] / a).max() > 0.9 * 2.0 ** -7
    assert (np.abs(p2.astype(np.float64))[normal] / a).max() > 0.9 * 2.0 ** -15


def test_non_finite_operands_leave_a_non_finite_piece():
    p = S.split3(np.array([np.inf, -np.inf, np.nan], dtype=np.float32))
    assert np.isinf(p[0][:2]).all() and np.isnan(p[1][:2]).all()                         # Inf - Inf: the split turns Inf into NaN
    assert np.isnan(p[0][2]) or np.isnan(p[1][2])


def test_dropped_terms_are_bounded_by_2_to_minus_21_and_carry_the_products_sign():
    bound = 2.0 ** -21 + 2.0 ** -30
    # per product, on random normal patterns within 2^+-30 (no under- or overflow of a piece product)
    rng = np.random.default_rng(2)
    n = 2_000_000
    def pat():
        u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        e = rng.integers(97, 158, n).astype(np.uint32)
        return _bits((u & np.uint32(0x807FFFFF)) | (e << np.uint32(23)))
    a, b = pat(), pat()
    pa = [p.astype(np.float64) for p in S.split3(a)]
    pb = [p.astype(np.float64) for p in S.split3(b)]
    prod = a.astype(np.float64) * b.astype(np.float64)
    drop = pa[1] * pb[2] + pa[2] * pb[1] + pa[2] * pb[2]
    keep = sum(pa[i] * pb[j] for i in range(3) for j in range(3) if i + j <= 2)
    assert (keep + drop == prod).all()                                                    # nine products of 8-bit pieces: exact in fp64
    ratio = np.abs(drop) / np.abs(prod)
    assert (ratio <= bound).all()
    assert (drop * np.sign(prod) >= 0).all()                                              # never against the product's sign
    assert (drop * np.sign(prod) > 0).mean() > 0.99
    print('\nrandom mantissas: max dropped/full = %.3f 2^-21, mean = 2^%.2f' % (ratio.max() * 2.0 ** 21, np.log2(ratio.mean())))
    assert 2.0 ** -25.5 < ratio.mean() < 2.0 ** -24                                       # (three terms of mean 1/4 2^-22, 1/4 2^-22, 2^-32)
    # per output element, on the adversarial pattern and on randn
    for M, N, K, P in S.ADVERSARIAL_CASES:
        x, w = S.adversarial_case(M, N, K, P)
        d, f, af = S.dropped(x, w), S.full(x, w), S.abs_full(x, w)
        assert (np.abs(d) <= bound * af).all()
        assert (d > 0).all()                                                              # all-positive operands: a bias, every output
        r = d / f
        print('adversarial %s: dropped/full in [%.3f, %.3f] 2^-21' % ((M, N, K, P), r.min() * 2.0 ** 21, r.max() * 2.0 ** 21))
        assert r.min() >= 0.9 * 2.0 ** -21
        assert np.allclose(S.kept(x, w) + d, f, rtol=K * 2.0 ** -52, atol=0)                  # (fp64 summation order only)
    x, w = rng.standard_normal((2, 70, 96)).astype(np.float32), rng.standard_normal((2, 128, 96)).astype(np.float32)
    assert (np.abs(S.dropped(x, w)) <= bound * S.abs_full(x, w)).all()


@pytest.mark.parametrize('case', S.EXACT_CASES, ids=lambda c: 'M%d_N%d_K%d_P%d' % c)
def test_exact_operands_make_every_partial_sum_representable(case):
    M, N, K, P = case
    (x, xp), (w, wp) = S.exact_case(M, N, K, P, with_pieces=True)
    assert x.shape == (P, M, K) and w.shape == (P, N, K)
    # the support: 16 positions per plane, shared by both operands, one in every K-step where the K-steps are at most 16
    nz = x != 0
    assert (nz.sum(-1) == S.EXACT_SUPPORT).all() and ((w != 0) == nz[:, :1, :]).all() and (nz == nz[:, :1, :]).all()
    if K // 16 <= S.EXACT_SUPPORT:
        assert nz[:, 0, :].reshape(P, K // 16, 16).any(-1).all()
    # the pieces are the intended ones, all three nonzero on the support
    for v, intended in ((x, xp), (w, wp)):
        for got, want in zip(S.split3(v), intended):
            assert np.array_equal(got, want)
            assert ((want != 0) == (v != 0)).all()
    # granule and magnitude: every kept product a multiple of 2^-18, their absolute sum below 2^24 granules
    a, b = [p.astype(np.float64) for p in xp], [p.astype(np.float64) for p in wp]
    sum_abs = np.zeros((P, M, N))
    for i in range(3):
        for j in range(3 - i):
            pr = a[i][:, :, None, :] * b[j][:, None, :, :] if M * N * K * P < 1 << 24 else None
            if pr is not None:
                assert (np.mod(pr, S.EXACT_GRANULE) == 0).all()
            else:                                                    # (the largest case: the granule through the pieces' lowest bits)
                assert S.low_bit(a[i]).min() * S.low_bit(b[j]).min() >= S.EXACT_GRANULE
            sum_abs += np.matmul(np.abs(a[i]), np.swapaxes(np.abs(b[j]), -1, -2))
    assert sum_abs.max() < S.EXACT_GRANULE * 2.0 ** 24
    k, f = S.kept(x, w), S.full(x, w)
    assert np.array_equal(k.astype(np.float32).astype(np.float64), k)                    # kept is an fp32 value
    assert np.array_equal(k + S.dropped(x, w), f)
    differs = (k.astype(np.float32) != f.astype(np.float32)).mean()
    print('\nkept != fp32(full) in %.1f %% of the outputs' % (100 * differs))
    assert differs >= 0.5                                                                 # a kernel that formed all nine products fails the GPU test


def test_scaling_cases_stay_inside_the_normal_range():
    x, w = S.scaling_case()
    K = x.shape[-1]
    assert (np.abs(x) >= 2.0 ** -4).all() and (np.abs(x) <= 2.0 ** 4).all() and (np.abs(w) >= 2.0 ** -4).all() and (np.abs(w) <= 2.0 ** 4).all()
    for s, t in [(0, 0)] + S.SCALINGS:
        xs, ws = np.ldexp(x, s), np.ldexp(w, t)
        assert np.array_equal(xs.astype(np.float64), np.ldexp(x.astype(np.float64), s))   # the scaling itself is exact
        assert np.array_equal(ws.astype(np.float64), np.ldexp(w.astype(np.float64), t))
        pa, pb = S.split3(xs), S.split3(ws)
        for scaled, plain, by in ((pa, S.split3(x), s), (pb, S.split3(w), t)):           # the pieces scale with the operand
            for p, q in zip(scaled, plain):
                assert np.array_equal(p.astype(np.float64), np.ldexp(q.astype(np.float64), by))
        la, lb = [S.low_bit(p).min() for p in pa], [S.low_bit(p).min() for p in pb]
        assert min(la + lb) >= 2.0 ** -126
        assert min(la[i] * lb[j] for i in range(3) for j in range(3 - i)) >= 2.0 ** -126  # the lowest bit of any kept product
        assert S.abs_full(xs, ws).max() < 2.0 ** 127                                      # >= sum |kept|: pieces never exceed the operand
    # the tiny case leaves that domain on purpose: pieces of x 2^-120 fall below 2^-126
    s, t = S.TINY_SCALING
    assert min(S.low_bit(p).min() for p in S.split3(np.ldexp(x, s))) < 2.0 ** -126
    assert K * 2.0 ** -126 * np.abs(np.ldexp(w, t)).max() < 2.0 ** -20 * np.abs(S.full(x, w)).max()      # the bound of the GPU test means something

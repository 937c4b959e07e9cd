"""The numpy model of detected beam power (helpers/beam_power_model.py; include/dcs_beam_power.h)
against exact rational arithmetic.  Where every p_t is a normal number, a block's P carries six roundings (square, add, four
levels) on non-negative terms, so it is within 6 * 2^-24 relative of the exact sum of re^2 + im^2 (the first-order bound;
the terms of second order are 2^-24 times smaller and the measured worst case leaves more than half the bound free); an
integration of n blocks adds at most n more.  Where squares are subnormal no bound is claimed: the model is the definition.
No GPU needed."""
from fractions import Fraction

import numpy as np

from helpers.beam_power_model import block_power, integrate, same_bits

U = Fraction(1, 2 ** 24)
TINY = float(np.finfo(np.float32).tiny)


def _exact_block(v):
    """v: [16][2] fp32 -> the exact sum of squares."""
    return sum(Fraction(float(x)) ** 2 for x in np.asarray(v, dtype=np.float32).ravel())


def _seeded(n_blocks, seed):
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3.0, np.log10(300.0), size=(n_blocks, 1, 1))
    return (rng.standard_normal((n_blocks, 16, 2)) * scale).astype(np.float32)


def test_block_power_is_within_six_roundings_of_the_exact_sum():
    v = _seeded(20000, 5)
    sq = (v * v).astype(np.float32)
    assert np.all((sq == 0) | (sq >= TINY)) and np.all((sq[..., 0] + sq[..., 1]) >= TINY)  # every p_t normal (or an exact 0 term)
    P = block_power(v.reshape(1, -1, 1, 16, 2))[0, :, 0]
    worst = Fraction(0)
    for i in range(v.shape[0]):
        exact = _exact_block(v[i])
        err = abs(Fraction(float(P[i])) - exact) / exact
        worst = max(worst, err)
    print(f"block: worst relative error {float(worst / U):.2f} units of 2^-24 over {v.shape[0]} blocks (bound 6)")
    assert worst <= 6 * U, float(worst / U)


def test_integration_is_within_n_more_roundings():
    for n, seed in ((2, 1), (16, 2), (5, 3)):
        groups = 20000 // 16 // n * n
        v = _seeded(groups * n, 40 + seed).reshape(groups, n, 16, 2)
        # [C = groups][nr_blocks = n][B = 1]
        P = block_power(v.reshape(groups, n, 1, 16, 2))
        S = integrate(P, n)[0, :, 0]
        worst = Fraction(0)
        for g in range(groups):
            exact = sum(_exact_block(v[g, j]) for j in range(n))
            worst = max(worst, abs(Fraction(float(S[g])) - exact) / exact)
        print(f"integration of {n}: worst relative error {float(worst / U):.2f} units of 2^-24 over {groups} spectra (bound {6 + n})")
        assert worst <= (6 + n) * U, (n, float(worst / U))


def test_integrate_orders_and_prior():
    rng = np.random.default_rng(9)
    P = rng.uniform(0.5, 2.0, size=(3, 12, 5)).astype(np.float32)
    one = integrate(P, 1)
    assert one.shape == (12, 3, 5) and np.array_equal(one, P.transpose(1, 0, 2))
    S = integrate(P, 4)
    assert S.shape == (3, 3, 5)
    for i in range(3):
        acc = P[:, 4 * i, :].copy()
        for j in range(1, 4):
            acc = (acc + P[:, 4 * i + j, :]).astype(np.float32)
        assert np.array_equal(S[i], acc)
    # a prior is the start of the chain: two halves with accumulate are the running sum, not the sum of two sums
    first = integrate(P[:, :6], 6)
    both = integrate(P[:, 6:], 6, prior=first)
    assert same_bits(both, integrate(P, 12)) is None
    assert both.shape == (1, 3, 5)


def test_tree_order_is_the_balanced_pairwise_one():
    """One large term and fifteen of half an ulp each: a left-to-right chain loses every small term (ties to even), the
    balanced tree collects them first.  Each order gives its own result, and the model gives the tree's."""
    half_ulp = np.float32(2.0 ** -24)  # half an ulp of 1
    p = np.full(16, half_ulp, dtype=np.float32)
    p[0] = 1.0
    v = np.zeros((1, 1, 1, 16, 2), dtype=np.float32)
    v[0, 0, 0, :, 0] = np.sqrt(p)  # 1 and 2^-12: exact squares
    assert np.array_equal((v[0, 0, 0, :, 0] ** 2).astype(np.float32), p)
    chain = np.float32(p[0])
    for t in range(1, 16):
        chain = np.float32(chain + p[t])
    assert chain == np.float32(1.0)
    # tree: level 1 (1 + h) = 1 (tie to even), the other pairs 2h; level 2: 1 + 2h = 1 + ulp; ...
    lvl = p.copy()
    while lvl.size > 1:
        lvl = (lvl[0::2] + lvl[1::2]).astype(np.float32)
    expected = np.float32(1.0) + np.float32(14 * 2.0 ** -24)
    assert lvl[0] == expected and expected != chain
    assert block_power(v)[0, 0, 0] == expected
    # the large term at another position changes which small term is lost, not the order of the tree
    v2 = np.roll(v, 5, axis=3)
    assert block_power(v2)[0, 0, 0] == expected
    # and a case that tells neighbours (0,1)(2,3) from a strided pairing (0,2)(1,3): p = [h, h, 1, 0, 0 ...]
    q = np.zeros(16, dtype=np.float32)
    q[0], q[1], q[2] = half_ulp, half_ulp, 1.0
    w = np.zeros((1, 1, 1, 16, 2), dtype=np.float32)
    w[0, 0, 0, :, 1] = np.sqrt(q)
    assert np.array_equal((w[0, 0, 0, :, 1] ** 2).astype(np.float32), q)
    neighbours = np.float32(np.float32(q[0] + q[1]) + np.float32(q[2] + q[3]))  # 2h + 1 = 1 + ulp
    strided = np.float32(np.float32(q[0] + q[2]) + np.float32(q[1] + q[3]))     # (h + 1 = 1) + h = 1
    assert neighbours == np.float32(1.0) + np.float32(2.0 ** -23) and strided == np.float32(1.0)
    assert block_power(w)[0, 0, 0] == neighbours


def test_subnormal_squares_are_kept_and_specials_follow_the_arithmetic():
    v = np.zeros((1, 1, 4, 16, 2), dtype=np.float32)
    v[0, 0, 0] = 1e-20   # squares 1e-40: subnormal
    v[0, 0, 1, 3, 1] = np.inf
    v[0, 0, 2, 7, 0] = np.nan
    P = block_power(v)[0, 0]
    sub = np.float32(np.float32(1e-20) * np.float32(1e-20))
    assert 0 < sub < TINY
    assert P[0] > 0 and Fraction(float(P[0])) == 32 * Fraction(float(sub))  # sums of subnormals are exact
    assert np.isposinf(P[1]) and np.isnan(P[2]) and P[3] == 0

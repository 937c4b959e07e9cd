"""The detector and integrator of include/dcs_beam_power.h in numpy fp32 alone: no GPU, no library.
Per sample p_t = RN(RN(re re) + RN(im im)); per 16-sample block the balanced pairwise sum of p_0 .. p_15 in sample order
(four levels, every add rounded once); an integration adds a spectrum's blocks in order, one rounded add each.  Every
operation below is a single numpy fp32 operation, which IEEE 754 rounds correctly and numpy does not flush.
tests/test_beam_power_model.py anchors it against exact rational arithmetic; tests/test_gpu_beam_power.py applies it to the
float call's output and compares the detecting kernels with it bit for bit."""
import numpy as np

F32 = np.float32


def block_power(v):
    """v: fp32 [C][nt/16][B][16][2] (the float beam tensor).  Returns fp32 [C][nt/16][B]."""
    v = np.asarray(v, dtype=F32)
    assert v.shape[-2:] == (16, 2), v.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        re, im = v[..., 0], v[..., 1]
        rr = (re * re).astype(F32)
        ii = (im * im).astype(F32)
        s = (rr + ii).astype(F32)  # p_t, [..][16]
        while s.shape[-1] > 1:     # neighbours (0, 1) (2, 3) ...
            s = (s[..., 0::2] + s[..., 1::2]).astype(F32)
    return s[..., 0]


def integrate(P, n, prior=None):
    """P: fp32 [C][nr_blocks][B]; n blocks per spectrum; prior: None or fp32 [nr_blocks / n][C][B] the sums start from.
    Returns fp32 [nr_blocks / n][C][B]."""
    P = np.asarray(P, dtype=F32)
    C, nb, B = P.shape
    assert n >= 1 and nb % n == 0, (nb, n)
    blocks = P.reshape(C, nb // n, n, B).transpose(1, 0, 2, 3)  # [i][c][j][b]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if prior is None:
            acc, first = blocks[:, :, 0, :].astype(F32).copy(), 1
        else:
            acc, first = np.asarray(prior, dtype=F32).reshape(nb // n, C, B).copy(), 0
        for j in range(first, n):
            acc = (acc + blocks[:, :, j, :]).astype(F32)
    return acc


def same_bits(got, exp):
    """None, or where the first difference is: finite values bit for bit, NaN positions equal, NaN payloads not compared."""
    got, exp = np.asarray(got, dtype=F32), np.asarray(exp, dtype=F32)
    if got.shape != exp.shape:
        return f"shapes differ: {got.shape} and {exp.shape}"
    gn, en = np.isnan(got), np.isnan(exp)
    bad = (gn != en) | (~en & ~gn & (got.view(np.uint32) != exp.view(np.uint32)))
    if not bad.any():
        return None
    i = np.unravel_index(int(np.flatnonzero(bad.ravel())[0]), got.shape)
    return f"{int(bad.sum())} of {got.size} values differ; first at {i}: got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), " \
           f"expected {exp[i]!r} ({exp.view(np.uint32)[i]:#010x})"

"""Anchors of the numpy model of the single-pulse search (helpers/single_pulse_model.py; include/dcs_single_pulse.h): the sums
and the peaks against plain Python loops over Python integers reduced mod 2^64 and mod 2^32, the signal-to-noise against
exact rationals rounded once per stated operation, and the chain whose numbers the GPU test relies on.  No GPU needed."""
import math
import struct
from fractions import Fraction

import numpy as np

from helpers.dedisperse_model import BAND_DESCENDING_64, DMS_40, dedisperse, dm_delays
from helpers.single_pulse_model import CHAIN, NO_TIME, chain_filterbank, nr_blocks_of, peaks, snr, sums, takes_part

M32, M64 = 1 << 32, 1 << 64


def rn64(q):
    """A rational rounded to the nearest double, ties to even, by explicit arithmetic on its integer significand (finite,
    normal results only)."""
    if q == 0:
        return 0.0
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -1022 <= e <= 1023
    scaled = q / Fraction(2) ** (e - 52)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return sign * math.ldexp(float(n), e - 52)


def sqrt64(x):
    """The correctly rounded square root of a double: math.sqrt, checked against the midpoints to its neighbours."""
    r = math.sqrt(x)
    lo, hi = Fraction(np.nextafter(r, 0.0)), Fraction(np.nextafter(r, np.inf))
    assert ((Fraction(r) + lo) / 2) ** 2 <= Fraction(x) <= ((Fraction(r) + hi) / 2) ** 2
    return r


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def seeded_plane(B, nr_dm, spectra, seed, top=1 << 20):
    return np.random.default_rng(seed).integers(0, top, size=(B, nr_dm, spectra), dtype=np.uint32)


def loop_peaks(plane, first, T, widths, max_width, block_len):
    """The contract as a triple loop over Python integers: {value, time} per (b, m, i, k)."""
    B, nr_dm, _ = plane.shape
    nb = nr_blocks_of(T, block_len)
    out = np.zeros((B, nr_dm, len(widths), nb, 2), np.uint32)
    for b in range(B):
        for m in range(nr_dm):
            row = [int(v) for v in plane[b, m]]
            for i, w in enumerate(widths):
                for k in range(nb):
                    if not 1 <= w <= max_width:
                        out[b, m, i, k] = (0, NO_TIME)
                        continue
                    best, at = -1, None
                    for t in range(k * block_len, min((k + 1) * block_len, T)):
                        s = sum(row[first + t:first + t + w]) % M32
                        if s > best:
                            best, at = s, t
                    out[b, m, i, k] = (best, at)
    return out


def test_sums_are_python_integer_sums_mod_2_64():
    plane = seeded_plane(2, 3, 50, seed=1, top=M32)
    plane[1, 2, 7] = plane[1, 2, 8] = M32 - 1
    got = sums(plane, 5, 40)
    for b in range(2):
        for m in range(3):
            s1 = s2 = 0
            for t in range(5, 45):
                x = int(plane[b, m, t])
                s1, s2 = s1 + x, s2 + x * x
            assert s2 >= M64 or (b, m) != (1, 2)  # the sum of squares does wrap where the two full words are
            assert (int(got[b, m, 0]), int(got[b, m, 1])) == (s1 % M64, s2 % M64)
    # accumulate: three calls are one
    acc = sums(plane, 5, 13)
    acc = sums(plane, 18, 0, out=acc)
    acc = sums(plane, 18, 20, out=acc)
    acc = sums(plane, 38, 7, out=acc)
    assert np.array_equal(acc, got) and got.dtype == np.uint64
    assert not sums(plane, 3, 0).any()


def test_peaks_are_the_loop_over_python_integers():
    widths = [3, 7, 1, 100, 7, 0, 101, NO_TIME]
    plane = seeded_plane(2, 3, 3 + 200 + 99, seed=2)
    got = peaks(plane, 3, 200, widths, 100, 64)
    assert got.shape == (2, 3, 8, 4, 2) and np.array_equal(got, loop_peaks(plane, 3, 200, widths, 100, 64))
    assert np.all(got[:, :, 5:, :, 0] == 0) and np.all(got[:, :, 5:, :, 1] == NO_TIME)
    assert np.array_equal(got[:, :, 1], got[:, :, 4]) and got[..., 1].min() == 0
    assert list(takes_part(widths, 100)) == [True] * 5 + [False] * 3
    # into a prefilled plane at first_block: the other blocks stay
    pre = np.full((2, 3, 8, 7, 2), 0x3C3C3C3C, np.uint32)
    into = peaks(plane, 3, 200, widths, 100, 64, out=pre, first_block=2)
    assert np.array_equal(into[:, :, :, 2:6], got) and np.all(into[:, :, :, :2] == 0x3C3C3C3C) and np.all(into[:, :, :, 6:] == 0x3C3C3C3C)


def test_peaks_wrap_like_python_integers_mod_2_32():
    # sums that pass 2^32: 4096 words of 255 * 32768; and every word 0xFFFFFFFF
    T, w = 70, 600
    for word in (8_355_840, M32 - 1):
        plane = np.full((1, 1, T + w - 1), word, np.uint32)
        got = peaks(plane, 0, T, [w, 1], w, 64)
        assert np.array_equal(got, loop_peaks(plane, 0, T, [w, 1], w, 64))
        assert np.all(got[0, 0, 0, :, 0] == (word * w) % M32) and list(got[0, 0, 0, :, 1]) == [0, 64]  # ties: the first t
    assert 8_355_840 * 4096 > M32
    # the prefix wraps, the sums do not
    plane = seeded_plane(1, 2, 130 + 4095, seed=3) + np.uint32(1 << 19)
    assert int(plane[0, 0].astype(np.uint64).sum()) > M32
    widths = [4096, 1, 64]
    got = peaks(plane, 0, 130, widths, 4096, 128)
    assert np.array_equal(got, loop_peaks(plane, 0, 130, widths, 4096, 128))
    # two equal maxima in one block: the earlier time
    plane = np.ones((1, 1, 300), np.uint32)
    plane[0, 0, [70, 200]] = 9
    got = peaks(plane, 0, 256, [1, 4], 4, 256)
    assert got[0, 0, 0, 0].tolist() == [9, 70] and got[0, 0, 1, 0].tolist() == [12, 67]


def fraction_snr(value, w, s1, s2, count):
    """include/dcs_single_pulse.h, one Fraction operation and one rounding per line."""
    N = rn64(Fraction(count))
    mean = rn64(Fraction(rn64(Fraction(s1))) / Fraction(N))
    q2 = rn64(Fraction(rn64(Fraction(s2))) / Fraction(N))
    mm = rn64(Fraction(mean) * Fraction(mean))
    var = rn64(Fraction(q2) - Fraction(mm))
    if not var > 0:
        return 0.0
    wm = rn64(Fraction(w) * Fraction(mean))
    num = rn64(Fraction(value) - Fraction(wm))
    den = sqrt64(rn64(Fraction(w) * Fraction(var)))
    return rn64(Fraction(num) / Fraction(den))


def test_snr_is_the_stated_sequence_of_roundings():
    T, widths, max_width = 300, [1, 5, 32, 33, 0, 5], 32
    plane = seeded_plane(2, 3, T + max_width - 1, seed=4)
    plane[1, 1] = 777  # no variance
    plane[0, 2] += np.uint32(0xFFF00000)  # sums past 2^53: the conversions to double round
    pk = peaks(plane, 0, T, widths, max_width, 128)
    sm = sums(plane, 0, T)
    assert int(sm[0, 2, 1]) > 1 << 53 or int(sm[0, 2, 0]) > 1 << 40
    got, best = snr(pk, widths, max_width, sm, T)
    assert got.dtype == np.float32 and got.shape == (2, 3, 6, 3) and best.shape == (2, 3, 3)
    for b in range(2):
        for m in range(3):
            for k in range(3):
                col = []
                for i, w in enumerate(widths):
                    if not 1 <= w <= max_width:
                        assert got[b, m, i, k] == -np.inf
                        col.append(-math.inf)
                        continue
                    exp = fraction_snr(int(pk[b, m, i, k, 0]), w, int(sm[b, m, 0]), int(sm[b, m, 1]), T)
                    assert bits32(got[b, m, i, k]) == bits32(exp), (b, m, i, k)
                    col.append(struct.unpack("<f", struct.pack("<f", exp))[0])
                assert best[b, m, k] == col.index(max(col))  # the lowest index of the largest
    assert not got[1, 1, :3].any() and np.all(best[1, 1] == 0)  # a constant series: 0 for every width, so the first
    assert np.array_equal(got[:, :, 1], got[:, :, 5]) and not np.any(best == 5)  # a duplicate width never wins
    # every width dropped, and no width at all
    _, none = snr(pk[:, :, 3:5], widths[3:5], max_width, sm, T)
    assert np.all(none == NO_TIME)
    _, none = snr(pk[:, :, :0], [], max_width, sm, T)
    assert np.all(none == NO_TIME)
    # a range of blocks into prefilled outputs
    pre, pre_best = np.full((2, 3, 6, 3), 7.0, np.float32), np.full((2, 3, 3), 9, np.uint32)
    part, part_best = snr(pk, widths, max_width, sm, T, first_block=1, nr_blocks=1, out=pre, best_out=pre_best)
    assert np.array_equal(part[:, :, :, 1], got[:, :, :, 1]) and np.all(part[:, :, :, [0, 2]] == 7.0)
    assert np.array_equal(part_best[:, :, 1], best[:, :, 1]) and np.all(part_best[:, :, [0, 2]] == 9)


def test_the_chain_recovers_the_injected_pulse():
    """What tests/test_gpu_single_pulse.py relies on, for the seeds 0 to 4: the largest signal-to-noise of the whole search
    lies at the injected DM, at the width of the pulse, in block 1 at time 500, well above everything away from that DM."""
    k = CHAIN
    table = dm_delays(k["C"], *BAND_DESCENDING_64, DMS_40)
    max_delay = int(table.max())
    T = k["outputs"] - k["max_width"] + 1
    for seed in range(5):
        fb = chain_filterbank(table, seed)
        plane = dedisperse(fb, table, 0, k["outputs"], max_delay)
        pk = peaks(plane, 0, T, k["widths"], k["max_width"], k["block_len"])
        sn, best = snr(pk, k["widths"], k["max_width"], sums(plane, 0, k["count"]), k["count"])
        at = np.unravel_index(np.argmax(sn), sn.shape)
        assert at == (0, k["dm_index"], 3, 1), (seed, at)
        assert pk[at][1] == k["row"] and best[0, k["dm_index"], 1] == 3
        assert 20.0 < sn[at] < 27.0
        far = np.delete(sn[0], np.arange(18, 23), axis=0)
        assert far.max() < 9.3 and np.sort(sn.ravel())[-2] < 18.0 < 23.0 < sn[at]  # the runner-up is about 17.4

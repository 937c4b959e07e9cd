"""Which compiled form a call of six kernels takes ("The forms" of sections 5.4, 5.11, 5.17, 5.18, 5.19, 5.20 and
5.22), restated on the CPU: the matrix-core beamformer's instantiation and geometry (bf_beamform_mfma.hip), the correlator's units (bf_correlator.hip), the incoherent beam's loads per row (bf_incoherent.hip), the
sifter's collapse of the width axis (bf_candidates.hip), the walk of the boxcar kernel's waves over (batch, block) pairs
(bf_single_pulse.hip), the grids of the two kernels whose workgroups walk their items (the correlator, bf_ddc.hip) and the
unrolled trips of the integrator (bf_integrate.hip).  Each launcher picks its form from the arguments alone, so a shape names
its form.  tests/test_launch_forms.py holds these rules to the kernels' source text and takes the census of the GPU tests'
tables (helpers/*_cases.py) with them."""

# ------------------------------------------------------------------------------------------------------------------ correlator

CORR_S = 4            # tiles along an edge of a unit: kS
CORR_SB = 2           # b tiles of a unit off the diagonal: kSB
CORR_WAVES = 4        # waves per workgroup, one item each
CORR_GRID = 1 << 20   # workgroups at most
CORR_MAX_A = 256


def correlator_plan(A):
    """(tiles, st, units) as bf_launch_correlate fills them."""
    tiles = (A + 15) // 16
    st = (tiles + CORR_S - 1) // CORR_S
    return tiles, st, st + st * (st - 1) // 2 * (CORR_S // CORR_SB)


def correlator_units(A):
    """[(diag, sa, NA)] of the units u = 0 .. units - 1 of one (channel, visibility), as the kernel decodes an item: the st
    squares on the diagonal first, then the squares below it, kS / kSB units each; NA = the a tiles that exist, kS at most."""
    tiles, st, units = correlator_plan(A)
    out = []
    for u in range(units):
        if u < st:
            out.append((True, u, min(tiles - u * CORR_S, CORR_S)))
            continue
        w = (u - st) // (CORR_S // CORR_SB)
        sa = 1
        while sa * (sa + 1) // 2 <= w:
            sa += 1
        out.append((False, sa, min(tiles - sa * CORR_S, CORR_S)))
    return out


def correlator_forms_that_exist(top=CORR_MAX_A):
    return {f for A in range(1, top + 1) for f in correlator_units(A)}


def correlator_grid(C, nr_vis, A):
    """(items, workgroups): a multiple of eight workgroups of four waves, 2^20 (rounded up to eight) at most."""
    items = C * nr_vis * correlator_plan(A)[2]
    blocks = (items + CORR_WAVES - 1) // CORR_WAVES
    return items, (min(blocks, CORR_GRID) + 7) & ~7


# ------------------------------------------------------------------------------------------------------------- incoherent beam

INCOH_LOADS = 8       # kLoads
INCOH_WAVES = 4
INCOH_GRID = 2048


def incoherent_form(A):
    """(NC, RPW): wave-wide loads per row, rows a wave carries at once."""
    NC = min((A + 31) // 32, 8)
    return NC, INCOH_LOADS // NC


# ------------------------------------------------------------------------------------------------------------ candidate sifter

def candidate_width_chain(nr_widths):
    """(chain, at): the take_widths<N> calls of one cell in order, as a tuple of N -- eights while eight widths are left, one
    four if four are left, then ones -- and for every width index the (position in the chain, j inside that call) at which it
    is compared."""
    chain, at, i = [], [], 0
    while i + 8 <= nr_widths:
        chain.append(8)
        i += 8
    if i + 4 <= nr_widths:
        chain.append(4)
        i += 4
    while i < nr_widths:
        chain.append(1)
        i += 1
    for pos, n in enumerate(chain):
        at += [(pos, j) for j in range(n)]
    assert len(at) == nr_widths == sum(chain)
    return tuple(chain), at


def chain_steps(chain):
    """What a chain presents to stage_tile's three loops: (the eights, the ordered pairs of consecutive calls)."""
    return chain.count(8), set(zip(chain, chain[1:]))


# ----------------------------------------------------------------------------------------------------------------- boxcar walk

BOXCAR_BATCH = 8      # kBatch
BOXCAR_WAVES = 4      # kWaves


def boxcar_walk(nr_widths, nb):
    """(walks, batches): per wave of a workgroup whose run has nb blocks, the (batch, block) pairs it takes, in order."""
    assert nr_widths >= 1 and nb >= 1
    batches = (nr_widths - 1) // BOXCAR_BATCH + 1
    walks = []
    for wave in range(BOXCAR_WAVES):
        batch, kb, seq = wave // nb, wave % nb, []
        while batch < batches:
            seq.append((batch, kb))
            next_batch, next_kb = batch, kb + BOXCAR_WAVES
            while next_kb >= nb:
                next_kb -= nb
                next_batch += 1
            batch, kb = next_batch, next_kb
        walks.append(seq)
    return walks, batches


def nb_class(nb):
    """1 .. 5 as they are; every larger run as 6: more blocks than waves, no wave skips a batch."""
    return min(nb, 6)


def boxcar_runs(T, block_len):
    """The nb of every workgroup of one series: runs of 4096 // block_len blocks."""
    run = 4096 // block_len
    nr_blocks = (T - 1) // block_len + 1
    return [min(run, nr_blocks - k) for k in range(0, nr_blocks, run)]


# ------------------------------------------------------------------------------------------------------------------------- DDC

DDC_SPAN = 512        # kSpanOut
DDC_GRID = 1 << 20


def ddc_grid(nr_inputs, nr_out):
    """(items, workgroups)."""
    items = nr_inputs * ((nr_out + DDC_SPAN - 1) // DDC_SPAN)
    return items, min(items, DDC_GRID)


# ------------------------------------------------------------------------------------------------------------------ integrator

INTEGRATE_UNROLL = {"f32": 4, "u32": 8, "i32": 8}


def integrate_trips(kind, n, accumulate):
    """(full unrolled trips capped at 2, tail length) of the lane's loop over its n words: the float loop starts at word 1
    unless it accumulates (word 0 is the start of the sum), the integer loops always at word 0."""
    count = n - (0 if accumulate or kind != "f32" else 1)
    unroll = INTEGRATE_UNROLL[kind]
    return min(count // unroll, 2), count % unroll


# ------------------------------------------------------------------------------------------------- matrix-core beamformer

BACC_WAVES = 4              # waves per workgroup of the product build
BACC_CHUNK = 64             # kKC: antennas per chunk
BACC_FP32_LDS_CAP = 26 * 1024
BACC_ENOUGH_INT8 = 5120     # waves that fill the chip once: 1280 four-wave workgroups
BACC_ENOUGH_FP32 = 4096     # workgroups
BACC_FLAGS = [(w, q, p, c) for w in (False, True) for q in (False, True) for p in (False, True) for c in (False, True) if not (q and p)]


def bacc_lds_bytes(nbt, A):
    """bacc_lds_bytes: the fp32 form's two coefficient planes, rows padded where tiles share them."""
    a_pad = (A + 3) & ~3
    ws = 16 * nbt + (16 if nbt > 1 else 0)
    return a_pad * ws * 2 * 4


def _wave_blocks(width, nbt, tpr):
    """The kernels' n_blocks of the four waves of a workgroup that owns ``width`` sample blocks, sorted."""
    out = []
    for wave in range(BACC_WAVES):
        slot = wave // nbt
        out.append((width - slot + tpr - 1) // tpr if width > slot else 0)
    return sorted(out)


def bacc_plan(A, B, C, nt, fp32_chain=False, weighted=False, quant=False, power=False, complex_=False):
    """bf_launch_beamform_acc for the product build (every probe knob 0), as a dict; None where it launches nothing (an empty
    tensor).  A refused call is an AssertionError.  ``fp32_chain`` is the launcher's `chain` (math_mode bit 3), and has
    nothing to do with the int8 form kChain, which is called "chain" here as in the kernel's FORM."""
    assert nt % 16 == 0
    nT16 = nt // 16
    if A == 0 or B == 0 or C == 0 or nT16 == 0:
        return None
    assert A <= 256, "not built"
    assert not (fp32_chain and (weighted or quant or power or complex_)) and not (quant and power), "refused"
    wide = not fp32_chain and A > 64
    staged = not fp32_chain and A <= 64
    nbt = 1 if wide else (4 if B > 32 else (2 if B > 16 else 1))
    nw = BACC_WAVES
    lds_of_four = bacc_lds_bytes(4, A)
    while fp32_chain and nbt > 1 and bacc_lds_bytes(nbt, A) > BACC_FP32_LDS_CAP:
        nbt >>= 1
    n_bgroups = (B + 16 * nbt - 1) // (16 * nbt)
    tpr = nw // nbt
    blocks_cap = 8 if staged and nbt == 4 and n_bgroups == 1 else 16
    max_rounds = 16 if fp32_chain else blocks_cap // tpr
    tiles = (nT16 + tpr - 1) // tpr * tpr
    if tiles > max_rounds * tpr:  # equal shares
        parts = (nT16 + max_rounds * tpr - 1) // (max_rounds * tpr)
        tiles = ((nT16 + parts - 1) // parts + tpr - 1) // tpr * tpr
    enough = BACC_ENOUGH_FP32 if fp32_chain else BACC_ENOUGH_INT8 // nw
    while tiles > tpr and C * n_bgroups * ((nT16 + tiles - 1) // tiles) < enough:
        tiles = ((tiles // tpr + 1) // 2) * tpr
    n_tgroups = (nT16 + tiles - 1) // tiles
    xcd_group = n_bgroups if wide else (n_bgroups if not fp32_chain and n_bgroups >= 16 else 1)
    grid = C * n_bgroups * n_tgroups
    assert grid <= 0x7fffffff
    assert not (quant and tiles // tpr > 126)  # (cannot be reached: rounds are 16 at the most)
    nop = 9 if complex_ else 6
    if fp32_chain:
        form, lds = "fp32", bacc_lds_bytes(nbt, A)
    elif staged:
        form, lds = "staged", (tiles * A * 32 + 1023) // 1024 * 1024
        if tpr > 1:
            lds += nbt * 4 * nop * 64 * 4
    else:
        form, lds = "chain", 4 * nop * 64 * 16 + 8 * 4 + (32 if quant else (16 if weighted else 0)) * 4
    last = nT16 - (n_tgroups - 1) * tiles
    return {"form": form, "full": A % 64 == 0, "nbt": nbt, "lds_of_four_tiles": lds_of_four, "tpr": tpr, "blocks_cap": blocks_cap,
            "tiles_per_wg": tiles, "n_tgroups": n_tgroups, "n_bgroups": n_bgroups, "xcd_group": xcd_group,
            "grid": grid, "block": 64 * nw, "lds": lds,
            "chunks": (A + BACC_CHUNK - 1) // BACC_CHUNK, "partial_chunk": A % BACC_CHUNK != 0,
            "blocks_full": _wave_blocks(min(tiles, nT16), nbt, tpr), "blocks_last": _wave_blocks(last, nbt, tpr)}


def bacc_instantiation(A, weighted=False, quant=False, power=False, complex_=False):
    """(FORM, FULL, W, Q, P, C): the instantiation of bf_beamform_i8_kernel that launch_i8 picks.  (The fp32 form's three
    instantiations are named by their plan's nbt.)"""
    assert not (quant and power) and 1 <= A <= 256
    return ("staged" if A <= 64 else "chain", A % 64 == 0, bool(weighted), bool(quant), bool(power), bool(complex_))


def bacc_instantiations_that_exist():
    return {(form, full) + flags for form in ("staged", "chain") for full in (False, True) for flags in BACC_FLAGS}


def bacc_depth(plan):
    """The most sample blocks the plan gives a wave."""
    return max(plan["blocks_full"][-1], plan["blocks_last"][-1])


def bacc_is_deep(plan):
    """A third block is a live second pair; the fp32 form has no pairs, its second block is its second trip."""
    return bacc_depth(plan) >= (2 if plan["form"] == "fp32" else 3)

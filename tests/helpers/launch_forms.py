"""Which compiled form a call of five kernels takes ("The forms" of sections 5.11, 5.17, 5.18, 5.19, 5.20 and 5.22),
restated on the CPU: the correlator's units (bf_correlator.hip), the incoherent beam's loads per row (bf_incoherent.hip), the
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

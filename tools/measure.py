#!/usr/bin/env python3
"""tools/measure.py -- the measurement scripts behind profiles/ and DESIGN.md, one CLI (needs an MI355X).

Nothing here is on the product path: every subcommand drives the library through the same ctypes C-ABI
the tests use.  The store-only studies need the probes build (include/dcs_probes.h):

    python tools/measure.py geometry --shapes cfg2,mid,cfg3,cfg4,narrow [--bits 32|16] [--sweep]
        default geometry vs dcs_bf_autotune vs an exhaustive sweep, per shape      -> profiles/r02_autotune.md
    python tools/measure.py refshape
        the reference's default tensor (64 x 64 x 16 x 256 steps): one launch, and the per-time-step
        launch shapes NAIVE / MULTIPLE_CHANNELS (a1 / a2)
    python tools/measure.py fp16 [--modes 0,4]
        fp16 generator rate per arithmetic form                                     -> profiles/r02_fp16.md
    python tools/measure.py fused
        fused generate + beamform rate on several shapes                            -> profiles/r0N_fused.md
    python tools/measure.py bfweights [--rounds 5]
        per-input beam weights: weighted against unweighted beamformer calls, alternating, in one process
                                                                                    -> profiles/r04_beam_weights.md
    python tools/measure.py bfq8 [--rounds 5] [--shape AxBxCxNT --variant float|q8|q8c]
        quantised int8 beam output: the float call against the int8 call (clip rate 0 and ~1 %, with and without
        counters), alternating, in one process; with DCS_LIB_PATH pointing at a -DDCS_Q8_DWORD_STORES build beside its
        companions, the other store form                                            -> profiles/r05_beam_quant.md
    python tools/measure.py bfpower [--rounds 5] [--shape AxBxCxNT --variant float|power|power+int]
        detected beam power: the float call (twice: its own spread) against the detecting call and the detecting call plus
        the integration, alternating, in one process                              -> profiles/r06_beam_power.md
    python tools/measure.py bfcomplex [--rounds 5] [--shape AxBxCxNT]
        the complex product: the float call (twice: its own spread), the complex float call plain and conjugated, the
        detecting call and the complex detecting call, alternating, in one process -> profiles/r10_beam_complex.md
    python tools/measure.py bfcq8 [--rounds 5] [--shape AxBxCxNT]
        8-bit voltage beams of the complex product: the complex float call (twice: its own spread), the complex int8 call
        and the element-wise int8 call, each without and with clip counters, alternating, in one process
        -> profiles/r11_beam_complex_quant.md
    python tools/measure.py incoh [--rounds 5] [--trace]
        the incoherent beam against the read probe (dcs_probe_reduce) over the same bytes and against the detecting call
        at 16 and 256 beams, alternating, in one process; --trace: a few launches of each kernel for
        `rocprofv3 --kernel-trace --stats -- python3 tools/measure.py incoh --trace`  -> profiles/r07_incoherent_beam.md
    python tools/measure.py stokes [--rounds 5]
        the Stokes detection of two polarisations' 8-bit beams at IQUV and at I against the incoherent beam over the same
        bytes (the same load pattern), alternating, in one process, and the integration  -> profiles/r12_stokes.md
    python tools/measure.py dedisperse [--rounds 5] [--shape CxDMSxTxB] [--direct-shape CxDMSxTxB]
        incoherent dedispersion of 8-bit filterbanks: time and byte-adds per second with the table dm_delays makes (the
        staged form) and, at a smaller shape, with a seeded random table of the same max_delay (the direct form), and
        the delay-table call                                                        -> profiles/r13_dedisperse.md
    python tools/measure.py single_pulse [--rounds 5] [--shape CxDMSxTxB] [--block-len 256] [--buffers 3]
        the single-pulse search on the planes of that shape: the sums, the boxcar peaks of 13 widths and the signal-to-noise,
        the peaks' share of one read of the planes, and all three against dedisperse_q8 in the same process
                                                                                    -> profiles/r14_single_pulse.md
    python tools/measure.py candidates [--rounds 5] [--shape CxDMSxTxB] [--block-len 64] [--threshold 6] [--max-candidates 4096]
        the candidate sifter on the signal-to-noise of that search: find_candidates on a plane with few candidates and with
        half the cells above the threshold, beside peak_snr and dedisperse_q8 in the same process
                                                                                    -> profiles/r17_candidates.md
    python tools/measure.py correlator [--rounds 5] [--shapes AxCxNTxN,...] [--buffers 2]
        the correlator's block call rotating over copies of the samples that together stay above the Infinity Cache, against
        the incoherent beam over the same bytes (the read yardstick), alternating, in one process: the time, the fraction of
        one read of the samples at 6.3 TB/s and the matrix cores' share at their peak rate, and the integration
                                                                                    -> profiles/r15_correlator.md
    python tools/measure.py ddc [--rounds 5] [--shape INPUTSxSAMPLES] [--trace]
        the digital down-converter at 128 inputs x 2^24 samples, 256 taps, with one band and with two, in turn in one process:
        the time, its fraction of one read of the samples plus the write of the outputs at 8 TB/s, and the matrix cores'
        share at their peak rate; --trace: a few launches only, for a counter run     -> profiles/r16_ddc.md
    python tools/measure.py channeliser [--rounds 5] [--shapes INPUTSxNxPxSPECTRA,...] [--trace]
        the polyphase channeliser's quantised and float calls per shape, in turn in one process on seeded float series of
        small integers, beside a device-to-device copy of the input's bytes in the same process: the time, the floor of the
        bytes it must move at 8 TB/s and the fraction of it reached; --trace: a few launches only, for a counter run
                                                                                    -> profiles/r18_channeliser.md
    python tools/measure.py rfi [--rounds 5] [--shapes BEAMSxSPECTRAxCHANNELSxBLOCK_LEN,...] [--nr-dm 512] [--trace]
        the RFI flagger's statistics pass, flags and cleaning per shape beside stokes_block over the same number of bytes, in
        turn in one process over two copies of the input: each time, its bytes' floor at 8 TB/s, its ratio to the yardstick, and
        the whole stage as a share of the dedispersion of the same spectra; --trace: a few launches only, for a counter run
                                                                                    -> profiles/r19_rfi.md
    python tools/measure.py fold [--rounds 5] [--shapes BEAMSxSPECTRAxCHANNELS,...] [--nbins 64,256,1024] [--subint-len 8192] [--dm 100]
        the pulsar folder per shape and nbin, with and without hits, beside fold_scrunch and dedisperse_q8 with one DM over the
        same window, in turn in one process over two copies of the input: each time, the fold's bytes' floor at 8 TB/s (window
        read once, profiles written once) and its ratio to the dedispersion; --trace: a few launches only
                                                                                    -> profiles/r20_fold.md
    python tools/measure.py fbank [--rounds 5] [--trace]
        8-bit search filterbanks: the quantiser and the sums against the read probe over the same input, alternating, in one
        process, and what the three calls add to a detected-beam pipeline; --trace as for incoh -> profiles/r08_filterbank.md
    python tools/measure.py bfreplay [--rounds 5] [--shape AxBxCxNT]
        the float matrix-core call made plainly (on a context that never captured), then replayed from a hipGraph and made
        plainly again, alternating, in one process: what a replay and the clearing of the class words cost; run once per
        build (DCS_LIB_PATH) to compare two                                        -> profiles/r09_class_words.md
    python tools/measure.py stream
        BASELINE configs[4]: full-tensor period and the largest slab at <= 200 us    -> profiles/r0N_streaming_config5.md
    python tools/measure.py stream --table-mode unchanged|host|device|staged-host|staged-host-pinned|staged-device ...
        the same per way of bringing a new delay table to EVERY tick (after autotune)  -> profiles/r04_streaming_staged.md
    python tools/measure.py pmc
        a few launches of each hot kernel, for `rocprofv3 --pmc ... -- python3 tools/measure.py pmc`
    python tools/measure.py sustained [--seconds 6]
        back-to-back launches at config 3 for several seconds (rate per second)
    DCS_LIB_PATH=probes/libdcs_probes.so python tools/measure.py stores --kind pattern|lean|kernel ...
        store-only probes and the real kernel with dcs_probe_knobs nomath / pace        -> profiles/r01_store_patterns.md
    python tools/measure.py sincos
        device sweep of the sincos forms over every fp32 in [1, 128)                 -> profiles/r01_sincos_ab.md
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from dc_sand_amd import BeamformerParameters, device  # noqa: E402
from dc_sand_amd.generator import SteeringCoefficientGenerator, simulate_input  # noqa: E402

SHAPES = {  # name: (ant, beams, chan, nt)
    "ref": (64, 16, 64, 256),
    "cfg2": (64, 64, 4096, 1),
    "mid": (64, 256, 8192, 1),
    "cfg3": (64, 1024, 32768, 1),
    "cfg4": (256, 512, 32768, 1),
    "narrow": (16, 16, 32768, 1),
    "wide": (64, 4096, 2048, 1),
    "small": (16, 64, 2048, 1),
    "small2": (64, 16, 512, 1),
    "small3": (16, 64, 4096, 1),
    "wide2": (256, 1024, 1024, 1),
}


def per_launch_ms(fn, settle_ms=30.0, timed_ms=12.0, stream=None, max_n=4000):
    """ms per call of ``fn`` at steady state: settle ~settle_ms on this access pattern (the first launches
    after a change of pattern run 3-10 % slow), then ONE event pair around ~timed_ms worth of calls."""
    e0, e1 = device.Event(), device.Event()
    fn()
    e0.record(stream)
    fn()
    fn()
    e1.record(stream)
    e1.synchronize()
    one = max(e1.elapsed_ms_since(e0) / 2, 1e-3)
    for _ in range(int(min(max_n, max(4, settle_ms / one)))):
        fn()
    n = int(min(max_n, max(4, timed_ms / one)))
    e0.record(stream)
    for _ in range(n):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e1.elapsed_ms_since(e0) / n


def make(shape, bits=32):
    A, B, C, nt = shape
    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(simulate_input(bp))
    bw = 1 if bits == 32 else 0
    nb = g.output_bytes(bw, nt)
    buf = device.mem_alloc(nb)
    return bp, g, bw, nb, buf


def cmd_geometry(args):
    rows = []
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        bp, g, bw, nb, buf = make(shape, args.bits)
        nt = shape[3]
        n = bp.coeffs_per_time_step() * nt
        run = lambda: g.generate(buf, nb, t0=1, nt=nt, bitwidth=bw)  # noqa: E731
        g.set_tuning()
        d = [per_launch_ms(run) for _ in range(2)]
        chosen = g.autotune(buf, nb, bitwidth=bw)
        a = [per_launch_ms(run) for _ in range(2)]
        g.set_tuning()
        d.append(per_launch_ms(run))
        g.set_tuning(**{k: chosen[k] for k in ("form", "tiles_per_block", "chan_per_block", "nontemporal", "wg_per_cu")})
        a.append(per_launch_ms(run))
        best = (1e9, None)
        table = []
        if args.sweep:
            cpbs = (4, 6, 8, 10, 11, 12, 13, 14, 16, 20, 24, 32) if args.bits == 32 else (16, 32, 64, 96, 128, 192, 256)
            for tpb, wpc in ((1, -1), (1, 7), (1, 6), (1, 5), (2, -1), (4, -1)):
                for cpb in cpbs:
                    g.set_tuning(form=args.form, tiles_per_block=tpb, chan_per_block=cpb, nontemporal=1, wg_per_cu=wpc)
                    ms = per_launch_ms(run, settle_ms=20.0, timed_ms=8.0)
                    table.append((ms, tpb, cpb, wpc))
                    if ms < best[0]:
                        best = (ms, (tpb, cpb, wpc))
            # second look at the five best (short trials rank neighbours only within their noise)
            top = sorted(table)[:5]
            best = (1e9, None)
            for _, tpb, cpb, wpc in top:
                g.set_tuning(form=args.form, tiles_per_block=tpb, chan_per_block=cpb, nontemporal=1, wg_per_cu=wpc)
                ms = min(per_launch_ms(run) for _ in range(2))
                if ms < best[0]:
                    best = (ms, (tpb, cpb, wpc))
        dm, am = min(d), min(a)
        line = (f"{name} {shape[0]}x{shape[1]}x{shape[2]} nt={nt} b{args.bits}: default {n / dm / 1e6:.1f}  autotuned {n / am / 1e6:.1f} "
                f"(tpb={chosen['tiles_per_block']} cpb={chosen['chan_per_block']} wg_per_cu={chosen['wg_per_cu']})")
        if best[1]:
            line += f"  sweep best {n / best[0] / 1e6:.1f} {best[1]}  default/best {best[0] / dm:.3f}  autotuned/default {dm / am:.3f}"
        print(line + "  Gcoeff/s", flush=True)
        if args.sweep and args.verbose:
            for ms, tpb, cpb, wpc in sorted(table)[:12]:
                print(f"    tpb={tpb} cpb={cpb:3d} wpc={wpc:2d}: {n / ms / 1e6:.1f}", flush=True)
        rows.append(dict(shape=name, dims=shape, bits=args.bits, default=n / dm / 1e6, autotuned=n / am / 1e6, chosen=chosen,
                         sweep_best=(n / best[0] / 1e6 if best[1] else None), sweep_best_geometry=best[1]))
        g.close()
        buf.free()
    print("JSON", json.dumps(rows), flush=True)


def cmd_refshape(args):
    """The tensor runBeamformerTests times (BeamformerParameters.h defaults): a3 in one launch, a1 / a2 as
    256 launches from the host loop (BeamformerCoefficientTest.cu:230-250); --sweep: a2 / a3 per geometry."""
    bp = BeamformerParameters()
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(simulate_input(bp))
    nt = 256
    nb = g.output_bytes(1, nt)
    buf = device.mem_alloc(nb)

    def t(kern, bw):
        nbb = g.output_bytes(bw, nt)
        return nbb, min(per_launch_ms(lambda: g.generate(buf, nbb, t0=0, nt=nt, kernel=kern, bitwidth=bw), settle_ms=20, timed_ms=40)
                        for _ in range(3))

    for kern, name in ((2, "MULTIPLE_CHANNELS_AND_TIMESTAMPS (1 launch)"), (1, "MULTIPLE_CHANNELS (256 launches)"), (0, "NAIVE (256 launches)")):
        for bw in ((1, 0) if kern else (1,)):
            nbb, ms = t(kern, bw)
            print(f"{name} b{32 if bw else 16}: {ms * 1e3:.1f} us per tensor = {ms * 1e3 / (nt if kern != 2 else 1):.2f} us per launch, "
                  f"{nbb / ms / 1e9:.2f} TB/s", flush=True)
    if args.sweep:
        for kern in (1, 2):
            for bw in (1, 0):
                for tpb in (1, 2, 4):
                    for cpb in (1, 2, 4, 8, 12, 16, 32, 64):
                        if cpb * tpb < 4:
                            continue
                        g.set_tuning(form=1, tiles_per_block=tpb, chan_per_block=cpb, wg_per_cu=-1)
                        nbb, ms = t(kern, bw)
                        print(f"  kernel={kern} b{32 if bw else 16} tpb={tpb} cpb={cpb:2d}: {ms * 1e3 / (nt if kern != 2 else 1):.2f} us per launch", flush=True)
    g.close()


def cmd_fp16(args):
    bp, g, _, _, buf = make(SHAPES["cfg3"], 32)
    n = bp.coeffs_per_time_step()
    bw = 1 if args.bits == 32 else 0
    nb16 = g.output_bytes(bw, 1)
    res = []
    for mode in [int(m) for m in args.modes.split(",")]:
        for tpb in [int(c) for c in args.tpb.split(",")]:
            for wpc in [int(c) for c in args.wpc.split(",")]:
                for cpb in [int(c) for c in args.cpb.split(",")]:
                    g.set_tuning(form=args.form, tiles_per_block=tpb, chan_per_block=cpb, nontemporal=1, math_mode=mode, wg_per_cu=wpc)
                    ms = min(per_launch_ms(lambda: g.generate(buf, nb16, t0=1, nt=1, bitwidth=bw)) for _ in range(2))
                    res.append((ms, mode, tpb, wpc, cpb))
                    print(f"fp16 math_mode={mode} tpb={tpb} cpb={cpb} wpc={wpc}: {ms:.4f} ms -> {n / ms / 1e6:.1f} Gcoeff/s = {nb16 / ms / 1e9:.2f} TB/s "
                          f"({nb16 / ms / 1e9 / 8 * 100:.1f} % of 8 TB/s)", flush=True)
    for mode in sorted({r[1] for r in res}):
        b = min(r for r in res if r[1] == mode)
        print(f"best math_mode={mode}: tpb={b[2]} cpb={b[4]} wpc={b[3]} -> {n / b[0] / 1e6:.1f} Gcoeff/s", flush=True)
    g.set_tuning(math_mode=int(args.modes.split(",")[-1]))
    ms = min(per_launch_ms(lambda: g.generate(buf, nb16, t0=1, nt=1, bitwidth=0)) for _ in range(2))
    print(f"library default geometry, math_mode={args.modes.split(',')[-1]}: {n / ms / 1e6:.1f} Gcoeff/s", flush=True)
    g.close()


def cmd_fused(args):
    for (A, B, C, nt) in ((64, 16, 64, 256), (64, 16, 4096, 256), (64, 64, 4096, 64), (64, 256, 4096, 16), (256, 64, 1024, 64)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, bb = A * C * nt * 2, B * C * nt * 8
        d_ant, d_beams = device.mem_alloc(ab), device.mem_alloc(bb)
        device.memset(d_ant, 3, ab)
        ms = per_launch_ms(lambda: g.generate_and_beamform(d_ant, ab, d_beams, bb, 0, nt))
        prods = A * B * C * nt
        print(f"{A}ant x {B}beam x {C}chan x {nt}t: fused {ms * 1e3:.1f} us -> {prods / ms / 1e6:.1f} G coefficient-products/s", flush=True)
        g.close()


def cmd_bfacc(args):
    """Beamformer with coefficient reuse on the matrix cores: rate against its roofline (int8 samples in + fp32 beams
    out vs 8 TB/s; fp32 MFMA 2 * 2 * A * B flop per sample vs 155 TFLOP/s)."""
    shapes = ((64, 16, 64, 256), (64, 16, 4096, 256), (64, 16, 4096, 4096), (64, 64, 4096, 256), (64, 256, 1024, 256), (256, 64, 1024, 256),
              (64, 1024, 256, 256))
    if args.shape:
        shapes = (tuple(int(v) for v in args.shape.split("x")),)
    for (A, B, C, nt) in shapes:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, bb = A * C * nt * 2, B * C * nt * 8
        d_ant, d_beams = device.mem_alloc(ab), device.mem_alloc(bb)
        if args.random:  # noise-like samples (what a telescope delivers): a 32 MiB seeded block repeated
            blk = min(ab, 32 << 20)
            device.memcpy_htod(d_ant, np.random.default_rng(0xA17).integers(-128, 128, size=blk, dtype=np.int8))
            off = blk
            while off < ab:
                n = min(off, ab - off)
                device.memcpy_dtod(int(d_ant) + off, d_ant, n)
                off += n
            device.synchronize()
        else:
            device.memset(d_ant, 3, ab)
        for mode in (int(m) for m in args.modes.split(",")):
            g.set_tuning(math_mode=mode)
            ms = min(per_launch_ms(lambda: g.beamform_accumulated(d_ant, ab, d_beams, bb, nt, t_coeff=1)) for _ in range(2))
            flop = 4.0 * A * B * C * nt
            form = "fp32 chain" if mode & 8 else "int8 fixed point"
            print(f"{A}ant x {B}beam x {C}chan x {nt}samples [{form}]: {ms * 1e3:.1f} us -> {A * B * C * nt / ms / 1e9:.2f} T coefficient-products/s, "
                  f"{(ab + bb) / ms / 1e9:.2f} TB/s algorithmic ({(ab + bb) / ms / 1e9 / 8 * 100:.1f} % of 8 TB/s), {flop / ms / 1e9:.1f} TFLOP/s-equivalent "
                  f"({flop / ms / 1e9 / 155 * 100:.1f} % of the fp32 MFMA peak)", flush=True)
        g.close()
        d_ant.free()
        d_beams.free()


def cmd_bfreplay(args):
    """One float call of the matrix-core beamformer per period, three ways: plain launches on a context that has never
    captured; the captured call replayed; plain launches after the capture (from then on every call of the context clears
    its class words: clear_class_words in bf_capi_beamform.hip)."""
    sys.path.insert(0, str(ROOT / "tests"))
    from helpers import hip_graph

    A, B, C, nt = (int(v) for v in args.shape.split("x"))
    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(simulate_input(bp))
    ab, bb = A * C * nt * 2, B * C * nt * 8
    d_ant, d_beams = device.mem_alloc(ab), device.mem_alloc(bb)
    _noise(d_ant, ab)
    s = device.Stream()

    def call():
        g.beamform_accumulated(d_ant, ab, d_beams, bb, nt, t_coeff=1, stream=s.handle)

    call()  # allocates
    s.synchronize()
    never = [per_launch_ms(call, stream=s.handle) * 1e3 for _ in range(args.rounds)]
    others = []
    nodes = hip_graph.launches(s, call, others)
    with hip_graph.capture(s) as graph:
        call()
    replay, after = [], []
    for _ in range(args.rounds):
        replay.append(per_launch_ms(lambda: graph.launch(s), stream=s.handle) * 1e3)
        after.append(per_launch_ms(call, stream=s.handle) * 1e3)
    graph.close()

    def line(name, v):
        print(f"{name}: median {sorted(v)[len(v) // 2]:.2f} us, min {min(v):.2f}, max {max(v):.2f}  ({', '.join(f'{x:.2f}' for x in v)})", flush=True)

    print(f"{A}ant x {B}beam x {C}chan x {nt}samples, float call; captured: {len(nodes)} kernel node(s), {len(others)} other node(s)", flush=True)
    line("plain, context never captured", never)
    line("replayed from the graph      ", replay)
    line("plain, after the capture     ", after)
    g.close()


def _noise(d_ant, nbytes):
    """Noise-like int8 samples (a 32 MiB seeded block repeated): the matrix pipe's power depends on the data."""
    blk = min(nbytes, 32 << 20)
    device.memcpy_htod(d_ant, np.random.default_rng(0xA17).integers(-128, 128, size=blk, dtype=np.int8))
    off = blk
    while off < nbytes:
        n = min(off, nbytes - off)
        device.memcpy_dtod(int(d_ant) + off, d_ant, n)
        off += n
    device.synchronize()


def cmd_bfweights(args):
    """Per-input beam weights (include/dcs_beam_weights.h): each shape's weighted and unweighted calls timed in turn,
    ``--rounds`` times each, in the same process on the same buffers; the median of each and their ratio."""
    from dc_sand_amd.beam_weights import BeamWeights

    cases = [("acc", s) for s in ((64, 16, 4096, 256), (64, 256, 4096, 256), (256, 64, 4096, 256))]
    cases += [("fused", s) for s in ((64, 16, 64, 256), (64, 16, 4096, 256), (64, 64, 4096, 64), (64, 256, 4096, 16), (256, 64, 1024, 64))]
    if args.shape:  # one shape (counter passes): AxBxCxNT, of --kind
        cases = [(args.kind, tuple(int(v) for v in args.shape.split("x")))]
    rows = []
    for kind, (A, B, C, nt) in cases:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, bb = A * C * nt * 2, B * C * nt * 8
        d_ant, d_beams = device.mem_alloc(ab), device.mem_alloc(bb)
        _noise(d_ant, ab)
        w = BeamWeights(bp)  # a taper with every eighth antenna flagged
        rng = np.random.default_rng(7)
        w.host[:] = rng.uniform(0.25, 1.0, size=w.host.shape).astype(np.float32)
        w.host[:, ::8] = 0.0
        w.upload()
        if kind == "acc":
            plain = lambda: g.beamform_accumulated(d_ant, ab, d_beams, bb, nt, t_coeff=1)  # noqa: E731
            weighted = lambda: g.beamform_accumulated_weighted(d_ant, ab, w.device_ptr(), d_beams, bb, nt, t_coeff=1)  # noqa: E731
            form = "staged" if A <= 64 else "kChain"
        else:
            plain = lambda: g.generate_and_beamform(d_ant, ab, d_beams, bb, 0, nt)  # noqa: E731
            weighted = lambda: g.generate_and_beamform_weighted(d_ant, ab, w.device_ptr(), d_beams, bb, 0, nt)  # noqa: E731
            form = "per-sample fused"
        t_plain, t_w = [], []
        for _ in range(args.rounds):
            t_plain.append(per_launch_ms(plain))
            t_w.append(per_launch_ms(weighted))
        mp, mw = float(np.median(t_plain)), float(np.median(t_w))
        row = {"kind": kind, "form": form, "shape": f"{A}x{B}x{C}x{nt}", "unweighted_us": round(mp * 1e3, 2),
               "weighted_us": round(mw * 1e3, 2), "ratio": round(mw / mp, 4),
               "spread_unweighted": round((max(t_plain) - min(t_plain)) / mp, 4), "spread_weighted": round((max(t_w) - min(t_w)) / mw, 4)}
        rows.append(row)
        print(f"{form:17s} {A}ant x {B}beam x {C}chan x {nt}t: unweighted {mp * 1e3:.1f} us, weighted {mw * 1e3:.1f} us, "
              f"ratio {mw / mp:.4f} (spread {row['spread_unweighted'] * 100:.1f} % / {row['spread_weighted'] * 100:.1f} %)", flush=True)
        w.free()
        g.close()
        d_ant.free()
        d_beams.free()
    print(json.dumps({"bfweights": rows}), flush=True)


def cmd_bfq8(args):
    """Quantised int8 beam output (include/dcs_beam_quant.h): per shape the float call (twice: its own spread) and the int8
    call at a clip rate of 0 and of about 1 %, each with and without counters, timed in turn ``--rounds`` times in the same
    process on the same buffers.  The gains come from the float output of the first channels; the clip rates printed are
    the counters' own.  ``--shape`` with ``--variant``: a few launches of one call only (counter passes)."""
    from dc_sand_amd.beam_quant import BeamQuantGains
    from dc_sand_amd.generator import quantised_beams_bytes

    shapes = [(64, 16, 32768, 256), (64, 256, 4096, 256), (256, 64, 4096, 256), (256, 64, 1024, 256)]
    if args.shape:
        shapes = [tuple(int(v) for v in args.shape.split("x"))]
    rows = []
    for A, B, C, nt in shapes:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, fb, qb = A * C * nt * 2, B * C * nt * 8, quantised_beams_bytes(bp, nt)
        d_ant, d_beams = device.mem_alloc(ab), device.mem_alloc(fb)
        d_q = device.mem_alloc(qb)
        _noise(d_ant, ab)
        f32 = lambda: g.beamform_accumulated(d_ant, ab, d_beams, fb, nt, t_coeff=1)  # noqa: E731
        f32()
        nc = min(C, 8)  # the gains: from the first channels' float beams
        v = np.empty((nc, nt // 16, B, 16, 2), dtype=np.float32)
        device.memcpy_dtoh(v, d_beams)
        mag = np.abs(np.moveaxis(v, 2, 0).reshape(B, -1)).astype(np.float64)
        sets = {}
        for name, k in (("0", 40.0 / mag.max(axis=1)), ("1pc", 127.5 / np.quantile(mag, 0.99, axis=1))):
            qg = BeamQuantGains(bp)
            qg.host[:] = k.astype(np.float32)
            qg.upload()
            sets[name] = qg

        def q8(name, count):
            qg = sets[name]
            return lambda: g.beamform_accumulated_q8(d_ant, ab, qg.device_ptr(), d_q, qb, nt, t_coeff=1,
                                                     d_clip_count=qg.clip_count_ptr() if count else None)
        rates = {}
        for name, qg in sets.items():  # the clip rate each gain set really gives, from one counted call
            q8(name, True)()
            rates[name] = float(qg.clip_counts(reset=True).sum()) / qb
        if args.shape:
            fn = {"float": f32, "q8": q8("1pc", False), "q8c": q8("1pc", True)}[args.variant]
            for _ in range(5):
                fn()
            device.synchronize()
            print(f"{args.variant} {A}x{B}x{C}x{nt}: algorithmic output bytes {fb if args.variant == 'float' else qb}", flush=True)
            return
        calls = [("float", f32), ("float_again", f32), ("q8_0", q8("0", False)), ("q8_0_counted", q8("0", True)),
                 ("q8_1pc", q8("1pc", False)), ("q8_1pc_counted", q8("1pc", True))]
        t = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, fn in calls:
                t[name].append(per_launch_ms(fn))
        med = {name: float(np.median(x)) for name, x in t.items()}
        spread = max(max(t["float"] + t["float_again"]) / min(t["float"] + t["float_again"]) - 1.0, abs(med["float_again"] / med["float"] - 1.0))
        row = {"shape": f"{A}x{B}x{C}x{nt}", "form": "staged" if A <= 64 else "kChain", "byte_ratio": round((2 * A + 2 * B) / (2 * A + 8 * B), 3),
               "float_us": round(med["float"] * 1e3, 1), "float_again_us": round(med["float_again"] * 1e3, 1), "float_spread": round(spread, 4),
               "float_frac_8TBps": round((2 * A + 8 * B) * C * nt / (med["float"] * 1e-3) / 8e12, 3),
               "clip_rate_0": rates["0"], "clip_rate_1pc": round(rates["1pc"], 5)}
        for name in ("q8_0", "q8_0_counted", "q8_1pc", "q8_1pc_counted"):
            row[name + "_us"] = round(med[name] * 1e3, 1)
            row[name + "_ratio"] = round(med[name] / med["float"], 4)
            row[name + "_frac_8TBps"] = round((2 * A + 2 * B) * C * nt / (med[name] * 1e-3) / 8e12, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        for qg in sets.values():
            qg.free()
        g.close()
        for d in (d_ant, d_beams, d_q):
            d.free()
    print(json.dumps({"bfq8": rows}), flush=True)


def cmd_bfpower(args):
    """Detected beam power (include/dcs_beam_power.h): per shape the float call (twice: its own spread), the detecting call,
    the detecting call followed by the integration of all its blocks into one spectrum, and the integration alone, timed in
    turn ``--rounds`` times in the same process on the same noise-like samples.  Bytes under the roofline's model: 2 A in
    and 8 B (float) or B / 4 (power) out per sample and channel.  ``--shape`` with ``--variant``: a few launches of one
    call only (counter passes)."""
    from dc_sand_amd.generator import block_power_bytes, power_spectra_bytes

    shapes = [(64, 16, 32768, 256), (64, 256, 4096, 256), (256, 64, 4096, 256), (256, 64, 1024, 256)]
    if args.shape:
        shapes = [tuple(int(v) for v in args.shape.split("x"))]
    rows = []
    for A, B, C, nt in shapes:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        nblk = nt // 16
        ab, fb, pb, sb = A * C * nt * 2, B * C * nt * 8, block_power_bytes(bp, nt), power_spectra_bytes(bp, nblk, nblk)
        d_ant, d_beams, d_p, d_s = device.mem_alloc(ab), device.mem_alloc(fb), device.mem_alloc(pb), device.mem_alloc(sb)
        _noise(d_ant, ab)
        f32 = lambda: g.beamform_accumulated(d_ant, ab, d_beams, fb, nt, t_coeff=1)  # noqa: E731
        power = lambda: g.beamform_accumulated_power(d_ant, ab, d_p, pb, nt, t_coeff=1)  # noqa: E731
        integ = lambda: g.integrate_block_power(d_p, pb, nblk, nblk, d_s, sb)  # noqa: E731

        def both():
            power()
            integ()
        f32()
        both()
        if args.shape:
            fn = {"float": f32, "power": power, "power+int": both}[args.variant]
            for _ in range(5):
                fn()
            device.synchronize()
            print(f"{args.variant} {A}x{B}x{C}x{nt}: algorithmic output bytes {fb if args.variant == 'float' else pb + (sb if args.variant == 'power+int' else 0)}",
                  flush=True)
            return
        calls = [("float", f32), ("float_again", f32), ("power", power), ("power_int", both), ("int", integ)]
        t = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, fn in calls:
                t[name].append(per_launch_ms(fn))
        med = {name: float(np.median(x)) for name, x in t.items()}
        spread = max(max(t["float"] + t["float_again"]) / min(t["float"] + t["float_again"]) - 1.0, abs(med["float_again"] / med["float"] - 1.0))
        bytes_f, bytes_p = (2 * A + 8 * B) * C * nt, (2 * A * 16 + 4 * B) * C * nblk
        row = {"shape": f"{A}x{B}x{C}x{nt}", "form": "staged" if A <= 64 else "kChain", "byte_ratio": round(bytes_p / bytes_f, 3),
               "float_us": round(med["float"] * 1e3, 1), "float_again_us": round(med["float_again"] * 1e3, 1), "float_spread": round(spread, 4),
               "float_frac_8TBps": round(bytes_f / (med["float"] * 1e-3) / 8e12, 3),
               "power_us": round(med["power"] * 1e3, 1), "power_ratio": round(med["power"] / med["float"], 4),
               "power_frac_8TBps": round(bytes_p / (med["power"] * 1e-3) / 8e12, 3),
               "power_int_us": round(med["power_int"] * 1e3, 1), "power_int_ratio": round(med["power_int"] / med["float"], 4),
               "int_us": round(med["int"] * 1e3, 1), "int_frac_8TBps": round((pb + sb) / (med["int"] * 1e-3) / 8e12, 3),
               "power_within_spread": bool(med["power"] <= med["float"] * (1.0 + spread))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        for d in (d_ant, d_beams, d_p, d_s):
            d.free()
    print(json.dumps({"bfpower": rows}), flush=True)


def cmd_bfcomplex(args):
    """The complex product (include/dcs_beam_complex.h) beside the element-wise calls of the same shape: per shape the float
    call (twice: its own spread), the complex float call plain and conjugated, the detecting call and the complex detecting
    call, timed in turn ``--rounds`` times in the same process on the same noise-like samples.  The bytes are the same in
    both forms; what differs is 24 matrix instructions per pair of blocks and 64 antennas instead of 12."""
    from dc_sand_amd.generator import block_power_bytes

    shapes = [(64, 16, 32768, 256), (64, 256, 4096, 256), (256, 64, 4096, 256), (256, 64, 1024, 256)]
    if args.shape:
        shapes = [tuple(int(v) for v in args.shape.split("x"))]
    rows = []
    for A, B, C, nt in shapes:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, fb, pb = A * C * nt * 2, B * C * nt * 8, block_power_bytes(bp, nt)
        d_ant, d_beams, d_p = device.mem_alloc(ab), device.mem_alloc(fb), device.mem_alloc(pb)
        _noise(d_ant, ab)
        calls = [("float", lambda: g.beamform_accumulated(d_ant, ab, d_beams, fb, nt, t_coeff=1)),
                 ("float_again", lambda: g.beamform_accumulated(d_ant, ab, d_beams, fb, nt, t_coeff=1)),
                 ("complex", lambda: g.beamform_accumulated_complex(d_ant, ab, d_beams, fb, nt, t_coeff=1)),
                 ("complex_conj", lambda: g.beamform_accumulated_complex(d_ant, ab, d_beams, fb, nt, t_coeff=1, conjugate=True)),
                 ("power", lambda: g.beamform_accumulated_power(d_ant, ab, d_p, pb, nt, t_coeff=1)),
                 ("complex_power", lambda: g.beamform_accumulated_complex_power(d_ant, ab, d_p, pb, nt, t_coeff=1, conjugate=True))]
        for _, fn in calls:
            fn()
        t = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, fn in calls:
                t[name].append(per_launch_ms(fn))
        med = {name: float(np.median(x)) for name, x in t.items()}
        spread = max(max(t["float"] + t["float_again"]) / min(t["float"] + t["float_again"]) - 1.0, abs(med["float_again"] / med["float"] - 1.0))
        row = {"shape": f"{A}x{B}x{C}x{nt}", "form": "staged" if A <= 64 else "kChain",
               "float_us": round(med["float"] * 1e3, 1), "float_again_us": round(med["float_again"] * 1e3, 1), "float_spread": round(spread, 4),
               "complex_us": round(med["complex"] * 1e3, 1), "complex_ratio": round(med["complex"] / med["float"], 4),
               "complex_conj_us": round(med["complex_conj"] * 1e3, 1), "complex_conj_ratio": round(med["complex_conj"] / med["float"], 4),
               "power_us": round(med["power"] * 1e3, 1), "complex_power_us": round(med["complex_power"] * 1e3, 1),
               "complex_power_ratio": round(med["complex_power"] / med["power"], 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        for d in (d_ant, d_beams, d_p):
            d.free()
    print(json.dumps({"bfcomplex": rows}), flush=True)


def cmd_bfcq8(args):
    """8-bit voltage beams of the complex product (include/dcs_beam_complex_quant.h): per shape the complex float call (twice:
    its own spread), the new call without and with clip counters, and the element-wise int8 call without and with them, all
    conjugated where they can be, timed in turn ``--rounds`` times in the same process on the same noise-like samples.  The gains put about 1 % of
    the components beyond the range (from the complex float output of the first channels); the clip rate printed is the
    counters' own.  Bytes under the roofline's model: 2 A in and 8 B (float) or 2 B (int8) out per sample and channel."""
    from dc_sand_amd.beam_quant import BeamQuantGains
    from dc_sand_amd.generator import quantised_beams_bytes

    shapes = [(64, 16, 32768, 256), (64, 256, 4096, 256), (256, 64, 4096, 256), (256, 64, 1024, 256)]
    if args.shape:
        shapes = [tuple(int(v) for v in args.shape.split("x"))]
    rows = []
    for A, B, C, nt in shapes:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, fb, qb = A * C * nt * 2, B * C * nt * 8, quantised_beams_bytes(bp, nt)
        d_ant, d_beams, d_q = device.mem_alloc(ab), device.mem_alloc(fb), device.mem_alloc(qb)
        _noise(d_ant, ab)
        cf32 = lambda: g.beamform_accumulated_complex(d_ant, ab, d_beams, fb, nt, t_coeff=1, conjugate=True)  # noqa: E731
        cf32()
        nc = min(C, 8)  # the gains: from the first channels' complex float beams
        v = np.empty((nc, nt // 16, B, 16, 2), dtype=np.float32)
        device.memcpy_dtoh(v, d_beams)
        mag = np.abs(np.moveaxis(v, 2, 0).reshape(B, -1)).astype(np.float64)
        qg = BeamQuantGains(bp)
        qg.host[:] = (127.5 / np.quantile(mag, 0.99, axis=1)).astype(np.float32)
        qg.upload()

        def cq8(count):
            return lambda: g.beamform_accumulated_complex_q8(d_ant, ab, qg.device_ptr(), d_q, qb, nt, t_coeff=1, conjugate=True,
                                                             d_clip_count=qg.clip_count_ptr() if count else None)

        def q8(count):
            return lambda: g.beamform_accumulated_q8(d_ant, ab, qg.device_ptr(), d_q, qb, nt, t_coeff=1,
                                                     d_clip_count=qg.clip_count_ptr() if count else None)
        cq8(True)()
        rate = float(qg.clip_counts(reset=True).sum()) / qb
        calls = [("cfloat", cf32), ("cfloat_again", cf32), ("cq8", cq8(False)), ("cq8_counted", cq8(True)), ("q8", q8(False)),
                 ("q8_counted", q8(True))]
        for _, fn in calls:
            fn()
        t = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, fn in calls:
                t[name].append(per_launch_ms(fn))
        med = {name: float(np.median(x)) for name, x in t.items()}
        both = t["cfloat"] + t["cfloat_again"]
        spread = max(max(both) / min(both) - 1.0, abs(med["cfloat_again"] / med["cfloat"] - 1.0))
        row = {"shape": f"{A}x{B}x{C}x{nt}", "form": "staged" if A <= 64 else "kChain", "byte_ratio": round((2 * A + 2 * B) / (2 * A + 8 * B), 3),
               "cfloat_us": round(med["cfloat"] * 1e3, 1), "cfloat_again_us": round(med["cfloat_again"] * 1e3, 1), "cfloat_spread": round(spread, 4),
               "clip_rate": round(rate, 5)}
        for name in ("cq8", "cq8_counted", "q8", "q8_counted"):
            row[name + "_us"] = round(med[name] * 1e3, 1)
        row["cq8_over_cfloat"] = round(med["cq8"] / med["cfloat"], 4)
        row["cq8_counted_over_cfloat"] = round(med["cq8_counted"] / med["cfloat"], 4)
        row["cq8_over_q8"] = round(med["cq8"] / med["q8"], 4)
        row["q8_counted_over_q8"] = round(med["q8_counted"] / med["q8"], 4)
        row["cq8_frac_8TBps"] = round((2 * A + 2 * B) * C * nt / (med["cq8"] * 1e-3) / 8e12, 3)
        row["cq8_within_spread"] = bool(med["cq8"] <= med["cfloat"] * (1.0 + spread))
        rows.append(row)
        print(json.dumps(row), flush=True)
        qg.free()
        g.close()
        for d in (d_ant, d_beams, d_q):
            d.free()
    print(json.dumps({"bfcq8": rows}), flush=True)


def cmd_incoh(args):
    """The incoherent beam (include/dcs_incoherent_beam.h), read-bound: 2 A bytes per sample and channel.  Per shape, in
    turn ``--rounds`` times in one process on the same noise-like samples: the new call (events around a run of launches),
    the read probe ``dcs_probe_reduce`` over the same bytes twice (its own spread; ONE event pair per call, because the
    probe call synchronises -- it also allocates and copies 128 KiB of partial sums back, which the events include, so
    the kernel-to-kernel comparison is the one of ``--trace``), the integration, and the detecting call at 16 and 256 beams.
    Inputs above the 256 MiB Infinity Cache are read from one buffer; the 128 MiB shape rotates over five buffers so that
    no call finds its lines cached.  ``--trace``: five launches of the new kernel and of the probe per shape, for a kernel
    trace's own durations."""
    from dc_sand_amd.generator import block_power_bytes, incoherent_block_power_bytes, incoherent_spectra_bytes
    from probes import dcs_probes as pr

    rows = []
    for A, C, nt, nbuf in [(64, 32768, 256, 1), (256, 4096, 256, 1), (64, 4096, 256, 5)]:
        nblk = nt // 16
        ab = A * C * nt * 2
        d_ants = [device.mem_alloc(ab) for _ in range(nbuf)]
        for d in d_ants:
            _noise(d, ab)
        turn = [0]

        def d_ant():
            turn[0] = (turn[0] + 1) % nbuf
            return d_ants[turn[0]]
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=16, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        pb, sb = incoherent_block_power_bytes(bp, nt), incoherent_spectra_bytes(bp, nblk, nblk)
        d_p, d_s = device.mem_alloc(pb), device.mem_alloc(sb)
        incoh = lambda: g.incoherent_block_power(d_ant(), ab, d_p, pb, nt)  # noqa: E731
        integ = lambda: g.integrate_incoherent_power(d_p, pb, nblk, nblk, d_s, sb)  # noqa: E731

        def probe_us():
            e0, e1 = device.Event(), device.Event()
            d = d_ant()
            e0.record()
            pr.tensor_properties(d, ab)
            e1.record()
            e1.synchronize()
            return e1.elapsed_ms_since(e0)
        incoh()
        integ()
        probe_us()
        if args.trace:
            for _ in range(5):
                incoh()
                device.synchronize()
                pr.tensor_properties(d_ant(), ab)
            print(f"trace {A}x{C}x{nt}: {ab} bytes read per launch of either kernel", flush=True)
        else:
            t = {name: [] for name in ("incoh", "probe", "probe_again", "int")}
            for _ in range(args.rounds):
                t["incoh"].append(per_launch_ms(incoh))
                t["probe"].append(float(np.median([probe_us() for _ in range(20)])))
                t["probe_again"].append(float(np.median([probe_us() for _ in range(20)])))
                t["int"].append(per_launch_ms(integ))
            med = {name: float(np.median(x)) for name, x in t.items()}
            both = t["probe"] + t["probe_again"]
            spread = max(max(both) / min(both) - 1.0, abs(med["probe_again"] / med["probe"] - 1.0))
            row = {"shape": f"{A}x{C}x{nt}", "input_MiB": ab >> 20, "buffers": nbuf,
                   "cache": "rotated" if nbuf > 1 else ("above the Infinity Cache" if ab > 256 << 20 else "cache-resident"),
                   "incoh_us": round(med["incoh"] * 1e3, 1), "incoh_TBps": round(ab / (med["incoh"] * 1e-3) / 1e12, 2),
                   "incoh_frac_8TBps": round(ab / (med["incoh"] * 1e-3) / 8e12, 3),
                   "probe_call_us": round(med["probe"] * 1e3, 1), "probe_call_again_us": round(med["probe_again"] * 1e3, 1),
                   "probe_call_TBps": round(ab / (med["probe"] * 1e-3) / 1e12, 2), "probe_spread": round(spread, 4),
                   "incoh_over_probe_call": round(med["incoh"] / med["probe"], 4), "int_us": round(med["int"] * 1e3, 1)}
        g.close()
        if not args.trace:  # what the incoherent beam adds to a detected-beam pipeline on the same samples
            for B in (16, 256):
                bpb = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
                gb = SteeringCoefficientGenerator(bpb)
                gb.upload_delays(simulate_input(bpb))
                dpb = block_power_bytes(bpb, nt)
                d_bp = device.mem_alloc(dpb)
                detect = lambda: gb.beamform_accumulated_power(d_ant(), ab, d_bp, dpb, nt, t_coeff=1)  # noqa: E731
                detect()
                ms = float(np.median([per_launch_ms(detect) for _ in range(args.rounds)]))
                row[f"bfpower_B{B}_us"] = round(ms * 1e3, 1)
                row[f"incoh_adds_to_B{B}"] = round(med["incoh"] / ms, 4)
                gb.close()
                d_bp.free()
            rows.append(row)
            print(json.dumps(row), flush=True)
        for d in d_ants + [d_p, d_s]:
            d.free()
    if not args.trace:
        print(json.dumps({"incoh": rows}), flush=True)


def cmd_stokes(args):
    """The Stokes detection of two polarisations' 8-bit beams (include/dcs_stokes.h), read-bound: per (beam, sample) 4 bytes
    read and 1 (IQUV) or 0.25 (I) written.  Per shape B x C x nt, in turn ``--rounds`` times in one process on the same
    noise-like bytes: the block call at IQUV and at I, the incoherent beam's block call over the very same bytes (x and y
    are the halves of one buffer, which a context of min(2 B, 256) antennas reads as one sample tensor: the yardstick,
    since it has the same load pattern), and the integration of the IQUV blocks.  Inputs above the 256 MiB Infinity
    Cache are read from one buffer; the shape that would fit rotates over three."""
    from dc_sand_amd.generator import (block_stokes_bytes, incoherent_block_power_bytes, quantised_beams_bytes,
                                       stokes_spectra_bytes)

    rows = []
    for B, C, nt, nbuf in [(16, 32768, 256, 1), (256, 4096, 256, 1), (64, 4096, 256, 3)]:
        nblk = nt // 16
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        qb = quantised_beams_bytes(bp, nt)
        bufs = [device.mem_alloc(2 * qb) for _ in range(nbuf)]
        for d in bufs:
            _noise(d, 2 * qb)
        turn = [0]

        def buf():
            turn[0] = (turn[0] + 1) % nbuf
            return int(bufs[turn[0]])
        g = SteeringCoefficientGenerator(bp)
        A = min(2 * B, 256)
        bpi = BeamformerParameters(NR_CHANNELS=C * 2 * B // A, NR_STATIONS=A, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=nt)
        gi = SteeringCoefficientGenerator(bpi)
        sb4, sb1 = block_stokes_bytes(bp, nt, 4), block_stokes_bytes(bp, nt, 1)
        pb, spb = incoherent_block_power_bytes(bpi, nt), stokes_spectra_bytes(bp, nblk, nblk, 4)
        d_bs, d_p, d_s = device.mem_alloc(sb4), device.mem_alloc(pb), device.mem_alloc(spb)

        def iquv():
            d = buf()
            g.stokes_block(d, d + qb, qb, d_bs, sb4, nt, nr_stokes=4)

        def only_i():
            d = buf()
            g.stokes_block(d, d + qb, qb, d_bs, sb1, nt, nr_stokes=1)
        incoh = lambda: gi.incoherent_block_power(buf(), 2 * qb, d_p, pb, nt)  # noqa: E731
        integ = lambda: g.integrate_stokes(d_bs, sb4, nblk, nblk, 4, d_s, spb)  # noqa: E731
        t = {name: [] for name in ("iquv", "i", "incoh", "incoh_again", "int")}
        for fn in (iquv, only_i, incoh, integ):
            fn()
        for _ in range(args.rounds):
            t["iquv"].append(per_launch_ms(iquv))
            t["incoh"].append(per_launch_ms(incoh))
            t["i"].append(per_launch_ms(only_i))
            t["incoh_again"].append(per_launch_ms(incoh))
        iquv()
        for _ in range(args.rounds):
            t["int"].append(per_launch_ms(integ))
        med = {name: float(np.median(x)) for name, x in t.items()}
        both = t["incoh"] + t["incoh_again"]
        tbps = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e12, 2)  # noqa: E731
        incoh_ms = float(np.median(both))
        row = {"shape": f"{B}x{C}x{nt}", "read_MiB": (2 * qb) >> 20, "buffers": nbuf,
               "cache": "rotated" if nbuf > 1 else "above the Infinity Cache",
               "iquv_us": round(med["iquv"] * 1e3, 1), "iquv_moved_TBps": tbps(2 * qb + sb4, med["iquv"]),
               "iquv_read_TBps": tbps(2 * qb, med["iquv"]),
               "i_us": round(med["i"] * 1e3, 1), "i_moved_TBps": tbps(2 * qb + sb1, med["i"]), "i_read_TBps": tbps(2 * qb, med["i"]),
               "incoh_us": round(incoh_ms * 1e3, 1), "incoh_read_TBps": tbps(2 * qb, incoh_ms),
               "incoh_spread": round(max(both) / min(both) - 1.0, 4),
               "iquv_read_rate_over_incoh": round(incoh_ms / med["iquv"], 4), "i_read_rate_over_incoh": round(incoh_ms / med["i"], 4),
               "iquv_moved_rate_over_incoh_read": round(incoh_ms / med["iquv"] * (2 * qb + sb4) / (2 * qb), 4),
               "int_us": round(med["int"] * 1e3, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        gi.close()
        for d in bufs + [d_bs, d_p, d_s]:
            d.free()
    print(json.dumps({"stokes": rows}), flush=True)


def cmd_dedisperse(args):
    """Incoherent dedispersion (include/dcs_dedisperse.h): nr_dm sums of C bytes per output sample, so B * nr_dm * T * C
    byte-adds per call.  A band of 1500 MHz down to 1200 MHz in C columns, 64 us spectra and DMs 0 .. 500: delays to about 8100
    spectra.  Noise-like bytes; ``--rounds`` timings of each call in one process.  The random table makes every chunk take the
    direct form, which reads every term from global memory: it is timed at a smaller shape."""
    from dc_sand_amd.generator import dm_delays_bytes, dm_time_bytes, filterbank_bytes

    def parse(text):
        C, nr_dm, T, B = (int(x) for x in text.lower().split("x"))
        return C, nr_dm, T, B
    rows = []
    for kind, (C, nr_dm, T, B) in (("dm_delays table", parse(args.shape)), ("random table", parse(args.direct_shape))):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
        g = SteeringCoefficientGenerator(bp)
        band = (1500.0, -300.0 / C, 64e-6)
        dms = np.linspace(0.0, 500.0, nr_dm)
        tb, pb = dm_delays_bytes(bp, nr_dm), dm_time_bytes(B, nr_dm, T)
        d_dms, d_delays, d_plane = device.mem_alloc(dms.nbytes), device.mem_alloc(tb), device.mem_alloc(pb)
        device.memcpy_htod(d_dms, dms)
        table_call = lambda: g.dm_delays(*band, d_dms, nr_dm, d_delays, tb)  # noqa: E731
        table_call()
        device.synchronize()
        table = np.empty((nr_dm, C), np.int32)
        device.memcpy_dtoh(table, d_delays)
        max_delay = int(table.max())
        t_table = [per_launch_ms(table_call) for _ in range(args.rounds)]
        if kind == "random table":
            table = np.random.default_rng(0xD15).integers(0, max_delay + 1, size=(nr_dm, C)).astype(np.int32)
            device.memcpy_htod(d_delays, table)
        in_spectra = T + max_delay
        fb = filterbank_bytes(bp, B, in_spectra)
        d_fb = device.mem_alloc(fb)
        _noise(d_fb, fb)
        call = lambda: g.dedisperse_q8(d_fb, fb, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_plane, pb, T)  # noqa: E731
        call()
        device.synchronize()
        t = [per_launch_ms(call, settle_ms=100.0, timed_ms=200.0) for _ in range(args.rounds)]
        ms = float(np.median(t))
        adds = B * nr_dm * T * C
        row = {"table": kind, "shape": f"C={C} nr_dm={nr_dm} T={T} B={B}", "max_delay": max_delay, "filterbank_MiB": fb >> 20,
               "ms": round(ms, 3), "spread": round(max(t) / min(t) - 1.0, 4), "byte_adds": adds,
               "byte_adds_per_s": float(f"{adds / (ms * 1e-3):.4g}"), "dm_delays_us": round(float(np.median(t_table)) * 1e3, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        for d in (d_dms, d_delays, d_plane, d_fb):
            d.free()
    print(json.dumps({"dedisperse": rows}), flush=True)


def cmd_single_pulse(args):
    """The single-pulse search (include/dcs_single_pulse.h) on the planes the dedispersion makes, at the shape of
    ``dedisperse``: 13 widths 1 .. 4096, blocks of 256 spectra.  The planes are made by dcs_bf_dedisperse_q8 from noise-like
    bytes, T + max_width - 1 words per series; that call is timed at T outputs in the same process.  boxcar_peaks and
    dm_time_sums are timed on one plane (which the Infinity Cache may hold, as it does right after the dedispersion) and
    rotating over ``--buffers`` copies that together exceed it; the bound is one read of the plane at 6.3 TB/s."""
    from dc_sand_amd.generator import (best_width_bytes, boxcar_peaks_bytes, dm_delays_bytes, dm_time_bytes, dm_time_sums_bytes,
                                       filterbank_bytes, peak_snr_bytes)

    C, nr_dm, T, B = (int(x) for x in args.shape.lower().split("x"))
    widths = np.array([1 << k for k in range(13)], np.uint32)
    max_width, block_len = 4096, args.block_len
    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
    g = SteeringCoefficientGenerator(bp)
    band = (1500.0, -300.0 / C, 64e-6)
    dms = np.linspace(0.0, 500.0, nr_dm)
    ps = T + max_width - 1
    tb, pb = dm_delays_bytes(bp, nr_dm), dm_time_bytes(B, nr_dm, ps)
    d_dms, d_delays, d_widths = device.mem_alloc(dms.nbytes), device.mem_alloc(tb), device.mem_alloc(widths.nbytes)
    planes = [device.mem_alloc(pb) for _ in range(args.buffers)]
    device.memcpy_htod(d_dms, dms)
    device.memcpy_htod(d_widths, widths)
    g.dm_delays(*band, d_dms, nr_dm, d_delays, tb)
    device.synchronize()
    table = np.empty((nr_dm, C), np.int32)
    device.memcpy_dtoh(table, d_delays)
    max_delay = int(table.max())
    in_spectra = ps + max_delay
    fb = filterbank_bytes(bp, B, in_spectra)
    d_fb = device.mem_alloc(fb)
    _noise(d_fb, fb)
    g.dedisperse_q8(d_fb, fb, in_spectra, 0, ps, B, d_delays, nr_dm, max_delay, planes[0], pb, ps)
    device.synchronize()
    for d in planes[1:]:
        device.memcpy_dtod(d, planes[0], pb)
    nb = (T + block_len - 1) // block_len
    sb, kb = dm_time_sums_bytes(B, nr_dm), boxcar_peaks_bytes(B, nr_dm, widths.size, nb)
    nbytes, bb = peak_snr_bytes(B, nr_dm, widths.size, nb), best_width_bytes(B, nr_dm, nb)
    d_sums, d_peaks, d_snr, d_best = (device.mem_alloc(n) for n in (sb, kb, nbytes, bb))
    turn = [0]

    def rotated(fn):
        def call():
            turn[0] = (turn[0] + 1) % len(planes)
            fn(planes[turn[0]])
        return call
    sums_on = lambda d: g.dm_time_sums(d, pb, ps, 0, T, B, nr_dm, d_sums, sb)  # noqa: E731
    peaks_on = lambda d: g.boxcar_peaks(d, pb, ps, 0, T, B, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kb, nb)  # noqa: E731
    snr_call = lambda: g.peak_snr(d_peaks, kb, nb, 0, nb, B, nr_dm, d_widths, widths.size, max_width, d_sums, sb, T, d_snr, nbytes,  # noqa: E731
                                  d_best, bb)
    dedisp = lambda: g.dedisperse_q8(d_fb, fb, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, planes[0], pb, ps)  # noqa: E731
    t = {k: [] for k in ("sums", "sums_rot", "peaks", "peaks_rot", "snr", "dedisperse")}
    for _ in range(args.rounds):
        t["peaks"].append(per_launch_ms(lambda: peaks_on(planes[0])))
        t["peaks_rot"].append(per_launch_ms(rotated(peaks_on)))
        t["sums"].append(per_launch_ms(lambda: sums_on(planes[0])))
        t["sums_rot"].append(per_launch_ms(rotated(sums_on)))
        t["snr"].append(per_launch_ms(snr_call))
        t["dedisperse"].append(per_launch_ms(dedisp, settle_ms=50.0, timed_ms=100.0))
    med = {k: float(np.median(v)) for k, v in t.items()}
    read = B * nr_dm * ps * 4
    bound_us = read / 6.3e12 * 1e6
    search_ms = med["sums"] + med["peaks"] + med["snr"]
    row = {"shape": f"C={C} nr_dm={nr_dm} T={T} B={B}", "widths": widths.size, "max_width": max_width, "block_len": block_len,
           "plane_read_MiB": read >> 20, "buffers": len(planes), "out_KiB": (kb + nbytes + bb + sb) >> 10,
           "peaks_us": round(med["peaks"] * 1e3, 1), "peaks_rotated_us": round(med["peaks_rot"] * 1e3, 1),
           "peaks_spread": round(max(t["peaks_rot"]) / min(t["peaks_rot"]) - 1.0, 4),
           "plane_read_bound_us": round(bound_us, 1), "peaks_rotated_share_of_bound": round(bound_us / (med["peaks_rot"] * 1e3), 3),
           "peaks_rotated_read_TBps": round(read / (med["peaks_rot"] * 1e-3) / 1e12, 2),
           "sums_us": round(med["sums"] * 1e3, 1), "sums_rotated_us": round(med["sums_rot"] * 1e3, 1),
           "sums_rotated_read_TBps": round(B * nr_dm * T * 4 / (med["sums_rot"] * 1e-3) / 1e12, 2),
           "snr_us": round(med["snr"] * 1e3, 1), "dedisperse_ms": round(med["dedisperse"], 3),
           "search_over_dedisperse": round(search_ms / med["dedisperse"], 4)}
    print(json.dumps({"single_pulse": row}), flush=True)
    g.close()
    for d in [d_dms, d_delays, d_widths, d_fb, d_sums, d_peaks, d_snr, d_best] + planes:
        d.free()


def cmd_candidates(args):
    """The candidate sifter (include/dcs_candidates.h) at the size of the search example: the signal-to-noise of 13 widths 1 ..
    4096 and blocks of ``--block-len`` spectra, made by the chain dedisperse_q8 -> dm_time_sums -> boxcar_peaks -> peak_snr
    from noise-like bytes.  find_candidates is timed at ``--threshold`` (on noise: few candidates, the scatter stages few
    tiles) and at threshold 0 (about half the cells at or above it: every tile is staged twice), beside peak_snr and
    dedisperse_q8 in the same process."""
    from dc_sand_amd.generator import (boxcar_peaks_bytes, candidates_bytes, candidates_workspace_bytes, dm_delays_bytes, dm_time_bytes,
                                       dm_time_sums_bytes, filterbank_bytes, peak_snr_bytes)

    C, nr_dm, T, B = (int(x) for x in args.shape.lower().split("x"))
    widths = np.array([1 << k for k in range(13)], np.uint32)
    max_width, block_len = 4096, args.block_len
    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
    g = SteeringCoefficientGenerator(bp)
    band = (1500.0, -300.0 / C, 64e-6)
    dms = np.linspace(0.0, 500.0, nr_dm)
    ps = T + max_width - 1
    tb, pb = dm_delays_bytes(bp, nr_dm), dm_time_bytes(B, nr_dm, ps)
    d_dms, d_delays, d_widths, d_plane = device.mem_alloc(dms.nbytes), device.mem_alloc(tb), device.mem_alloc(widths.nbytes), device.mem_alloc(pb)
    device.memcpy_htod(d_dms, dms)
    device.memcpy_htod(d_widths, widths)
    g.dm_delays(*band, d_dms, nr_dm, d_delays, tb)
    device.synchronize()
    table = np.empty((nr_dm, C), np.int32)
    device.memcpy_dtoh(table, d_delays)
    max_delay = int(table.max())
    in_spectra = ps + max_delay
    fb = filterbank_bytes(bp, B, in_spectra)
    d_fb = device.mem_alloc(fb)
    _noise(d_fb, fb)
    nb = (T + block_len - 1) // block_len
    sb, kb, nbytes = dm_time_sums_bytes(B, nr_dm), boxcar_peaks_bytes(B, nr_dm, widths.size, nb), peak_snr_bytes(B, nr_dm, widths.size, nb)
    cap = args.max_candidates
    cb, wb = candidates_bytes(cap), candidates_workspace_bytes(B, nr_dm, nb)
    d_sums, d_peaks, d_snr, d_cands, d_count, d_work = (device.mem_alloc(n) for n in (sb, kb, nbytes, cb, 8, wb))
    dedisp = lambda: g.dedisperse_q8(d_fb, fb, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_plane, pb, ps)  # noqa: E731
    snr_call = lambda: g.peak_snr(d_peaks, kb, nb, 0, nb, B, nr_dm, d_widths, widths.size, max_width, d_sums, sb, T, d_snr, nbytes)  # noqa: E731
    g.dedisperse_q8(d_fb, fb, in_spectra, 0, ps, B, d_delays, nr_dm, max_delay, d_plane, pb, ps)
    g.dm_time_sums(d_plane, pb, ps, 0, T, B, nr_dm, d_sums, sb)
    g.boxcar_peaks(d_plane, pb, ps, 0, T, B, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kb, nb)
    snr_call()

    def find(threshold):
        return lambda: g.find_candidates(d_snr, nbytes, d_peaks, kb, nb, 0, nb, B, nr_dm, widths.size, threshold, args.dm_radius,
                                         args.block_radius, d_cands, cb, cap, d_count, d_work, wb)
    found = {}
    count = np.empty(2, np.uint32)
    for name, threshold in (("sparse", args.threshold), ("dense", 0.0)):
        find(threshold)()
        device.synchronize()
        device.memcpy_dtoh(count, d_count)
        found[name] = count.tolist()
    t = {k: [] for k in ("sparse", "dense", "snr", "dedisperse")}
    for _ in range(args.rounds):
        t["sparse"].append(per_launch_ms(find(args.threshold)))
        t["dense"].append(per_launch_ms(find(0.0)))
        t["snr"].append(per_launch_ms(snr_call))
        t["dedisperse"].append(per_launch_ms(dedisp, settle_ms=50.0, timed_ms=100.0))
    med = {k: float(np.median(v)) for k, v in t.items()}
    row = {"shape": f"C={C} nr_dm={nr_dm} T={T} B={B}", "widths": widths.size, "block_len": block_len, "blocks": nb,
           "snr_MiB": round(nbytes / 2**20, 1), "workspace_KiB": wb >> 10, "radii": [args.dm_radius, args.block_radius],
           "max_candidates": cap, "threshold": args.threshold, "found": found["sparse"], "found_at_threshold_0": found["dense"],
           "find_candidates_us": round(med["sparse"] * 1e3, 1),
           "find_candidates_spread": round(max(t["sparse"]) / min(t["sparse"]) - 1.0, 4),
           "find_candidates_at_threshold_0_us": round(med["dense"] * 1e3, 1),
           "snr_read_TBps": round(nbytes / (med["sparse"] * 1e-3) / 1e12, 2),
           "peak_snr_us": round(med["snr"] * 1e3, 1), "dedisperse_ms": round(med["dedisperse"], 3),
           "find_candidates_over_dedisperse": round(med["sparse"] / med["dedisperse"], 5)}
    print(json.dumps({"candidates": row}), flush=True)
    g.close()
    for d in (d_dms, d_delays, d_widths, d_plane, d_fb, d_sums, d_peaks, d_snr, d_cands, d_count, d_work):
        d.free()


def cmd_correlator(args):
    """The correlator (include/dcs_correlator.h): one read of the samples (A * 32 bytes per channel and block) and
    NB * 8 bytes written per channel and visibility.  Per shape A x C x nt x n, in turn ``--rounds`` times in one process on the
    same noise-like samples: the block call and the incoherent beam's block call over the very same bytes (a streaming read
    of the same tensor: the yardstick), each rotating over ``--buffers`` copies, and the integration of all visibilities of a
    channel.  The bound is one read of the samples at 6.3 TB/s; the matrix cores' time is 4 MFMAs of 16x16x64 i8 per tile
    pair and four blocks at 16 cycles each on 1024 SIMDs at 2.4 GHz."""
    from dc_sand_amd.generator import block_visibilities_bytes, incoherent_block_power_bytes, nr_baselines, visibilities_bytes

    rows = []
    for shape in args.shapes.split(","):
        A, C, nt, n = (int(x) for x in shape.split("x"))
        nblk, nr_vis = nt // 16, nt // 16 // n
        ab = A * C * nt * 2
        nbuf = max(args.buffers, -(-(512 << 20) // ab))  # together at least twice the Infinity Cache
        bufs = [device.mem_alloc(ab) for _ in range(nbuf)]
        for d in bufs:
            _noise(d, ab)
        turn = [0]

        def d_ant():
            turn[0] = (turn[0] + 1) % nbuf
            return bufs[turn[0]]
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        vb, ob, pb = block_visibilities_bytes(bp, nt, n), visibilities_bytes(bp, nr_vis, nr_vis), incoherent_block_power_bytes(bp, nt)
        d_vis, d_out, d_p = device.mem_alloc(vb), device.mem_alloc(ob), device.mem_alloc(pb)
        corr = lambda: g.correlate_block(d_ant(), ab, d_vis, vb, nt, n)  # noqa: E731
        incoh = lambda: g.incoherent_block_power(d_ant(), ab, d_p, pb, nt)  # noqa: E731
        integ = lambda: g.integrate_visibilities(d_vis, vb, nr_vis, nr_vis, d_out, ob)  # noqa: E731
        for fn in (corr, incoh, integ):
            fn()
        t = {name: [] for name in ("corr", "incoh", "incoh_again", "int")}
        for _ in range(args.rounds):
            t["corr"].append(per_launch_ms(corr))
            t["incoh"].append(per_launch_ms(incoh))
            t["incoh_again"].append(per_launch_ms(incoh))
            t["int"].append(per_launch_ms(integ))
        med = {name: float(np.median(x)) for name, x in t.items()}
        both = t["incoh"] + t["incoh_again"]
        incoh_ms = float(np.median(both))
        tiles = -(-A // 16)
        mfmas = tiles * (tiles + 1) // 2 * 4 * C * nr_vis * -(-n // 4)
        mfma_ms = mfmas * 16 / (1024 * 2.4e9) * 1e3
        bound_ms = ab / 6.3e12 * 1e3
        row = {"shape": shape, "baselines": nr_baselines(A), "read_MiB": ab >> 20, "written_MiB": round(vb / (1 << 20), 1),
               "buffers": nbuf, "corr_us": round(med["corr"] * 1e3, 1), "corr_spread": round(max(t["corr"]) / min(t["corr"]) - 1.0, 4),
               "corr_read_TBps": round(ab / (med["corr"] * 1e-3) / 1e12, 2),
               "read_bound_us": round(bound_ms * 1e3, 1), "frac_of_read_bound": round(bound_ms / med["corr"], 3),
               "mfma_peak_us": round(mfma_ms * 1e3, 1), "mfma_share_of_time": round(mfma_ms / med["corr"], 3),
               "incoh_us": round(incoh_ms * 1e3, 1), "incoh_read_TBps": round(ab / (incoh_ms * 1e-3) / 1e12, 2),
               "incoh_spread": round(max(both) / min(both) - 1.0, 4), "corr_over_incoh": round(med["corr"] / incoh_ms, 3),
               "int_us": round(med["int"] * 1e3, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        for d in bufs + [d_vis, d_out, d_p]:
            d.free()
    print(json.dumps({"correlator": rows}), flush=True)


def cmd_ddc(args):
    """The digital down-converter (include/dcs_ddc.h): one read of the samples and nr_bands * 8 bytes written per 16 of them.
    At ``--shape`` inputs x samples with 256 random taps of full digit range (the time does not depend on their values), one
    band and two in turn, ``--rounds`` times in one process on the same noise-like samples.  The bound is the read plus the
    write at 8 TB/s; the matrix cores' time is one MFMA of 16x16x64 i8 per 64 taps and 16 outputs at 16 cycles each on
    1024 SIMDs at 2.4 GHz (the same count for one band and two: a band is a set of rows of the operand)."""
    from dc_sand_amd.generator import ddc_digits_bytes, ddc_out_bytes

    ni, n = (int(x) for x in args.shape.split("x"))
    T = 256
    nr_out = (n - T) // 16 + 1
    g = SteeringCoefficientGenerator(BeamformerParameters(NR_CHANNELS=1, NR_STATIONS=1, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=16))
    d_x = device.mem_alloc(ni * n)
    _noise(d_x, ni * n)
    d_out = device.mem_alloc(ddc_out_bytes(ni, nr_out, 2))
    taps = np.random.default_rng(16).integers(-60000, 60001, size=(2, T, 2)).astype(np.int32)
    d_taps, d_digits = device.mem_alloc(taps.nbytes), [device.mem_alloc(ddc_digits_bytes(T)) for _ in range(2)]
    device.memcpy_htod(d_taps, taps)
    bands = [(250609664, 0, 1e-6), (0x3579BDF1, 7, 2e-6)]
    calls = {}
    for nb in (1, 2):
        g.ddc_tap_digits(d_taps, T, nb, d_digits[nb - 1], ddc_digits_bytes(T))
        calls[nb] = (lambda nb=nb: g.ddc(d_x, ni * n, n, ni, nr_out, d_digits[nb - 1], ddc_digits_bytes(T), T, bands[:nb], d_out,
                                         ddc_out_bytes(ni, nr_out, nb), nr_out))
    device.synchronize()
    if args.trace:
        for _ in range(3):
            for nb in (1, 2):
                calls[nb]()
        device.synchronize()
        return
    t = {1: [], 2: []}
    for _ in range(args.rounds):
        for nb in (1, 2):
            t[nb].append(per_launch_ms(calls[nb]))
    rows = []
    for nb in (1, 2):
        ms = float(np.median(t[nb]))
        moved = ni * n + ddc_out_bytes(ni, nr_out, nb)
        mfma_ms = ni * -(-nr_out // 16) * (T // 64) * 16 / (1024 * 2.4e9) * 1e3
        rows.append({"shape": args.shape, "taps": T, "bands": nb, "nr_out": nr_out, "read_MiB": ni * n >> 20,
                     "written_MiB": ddc_out_bytes(ni, nr_out, nb) >> 20, "us": round(ms * 1e3, 1),
                     "spread": round(max(t[nb]) / min(t[nb]) - 1.0, 4), "moved_TBps": round(moved / (ms * 1e-3) / 1e12, 2),
                     "bound_us_at_8TBps": round(moved / 8e12 * 1e6, 1), "frac_of_bound": round(moved / 8e12 * 1e3 / ms, 3),
                     "mfma_peak_us": round(mfma_ms * 1e3, 1), "mfma_share_of_time": round(mfma_ms / ms, 3),
                     "Gsamples_per_s": round(ni * n / (ms * 1e-3) / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"ddc": rows}), flush=True)
    g.close()
    for d in [d_x, d_out, d_taps] + d_digits:
        d.free()


def cmd_channeliser(args):
    """The polyphase channeliser (include/dcs_channeliser.h).  Per shape (inputs x N x P x spectra) the quantised call, the
    float call and a device-to-device copy of the input's bytes (the copy figure of the same session), in turn ``--rounds``
    times in one process.  The floor is the bytes the call must move -- inputs (spectra + P - 1) N 8 read, inputs spectra N 2
    (int8) or 8 (float) written -- at the 8 TB/s HBM peak.  The input is a seeded series of small integers as floats (a 32 MiB
    block repeated), the taps pfb_taps, the gains 2^-3: the time does not depend on the values."""
    from dc_sand_amd import _lib, channeliser
    from dc_sand_amd.generator import channelised_bytes, channeliser_in_pairs

    g = SteeringCoefficientGenerator(BeamformerParameters(NR_CHANNELS=1, NR_STATIONS=1, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=16))
    rows = []
    for shape in args.shapes.split(","):
        ni, N, P, ns = (int(x) for x in shape.split("x"))
        pairs = channeliser_in_pairs(N, P, ns)
        in_bytes, fbytes, qbytes = ni * pairs * 8, channelised_bytes(N, ns // 16, ni), channelised_bytes(N, ns // 16, ni, q8=True)
        d_in, d_f, d_q = device.mem_alloc(in_bytes), device.mem_alloc(max(fbytes, in_bytes)), device.mem_alloc(qbytes)
        blk = min(in_bytes, 32 << 20)
        device.memcpy_htod(d_in, np.random.default_rng(18).integers(-100, 101, size=blk // 4).astype(np.float32))
        off = blk
        while off < in_bytes:
            n = min(off, in_bytes - off)
            device.memcpy_dtod(int(d_in) + off, d_in, n)
            off += n
        taps, tw = channeliser.pfb_taps(N, P), channeliser.twiddles(N)
        gains = np.full((ni, N), 0.125, dtype=np.float32)
        d_taps, d_tw, d_g, d_n = (device.mem_alloc(b) for b in (taps.nbytes, tw.nbytes, gains.nbytes, 8 * ni))
        device.memcpy_htod(d_taps, taps)
        device.memcpy_htod(d_tw, tw)
        device.memcpy_htod(d_g, gains)
        device.memset(d_n, 0, 8 * ni)
        calls = {
            "q8": lambda: g.channelise_q8(d_in, in_bytes, pairs, ni, ns, N, P, d_taps, d_tw, d_g, d_q, qbytes, ns // 16, ni, d_clip_count=d_n),
            "float": lambda: g.channelise(d_in, in_bytes, pairs, ni, ns, N, P, d_taps, d_tw, d_f, fbytes, ns // 16, ni),
            "copy": lambda: _lib.check(_lib.lib().dcs_memcpy_dtod(ctypes.c_void_p(int(d_f)), ctypes.c_void_p(int(d_in)), in_bytes, None), "dtod"),
        }
        device.synchronize()
        if args.trace:
            for _ in range(3):
                calls["q8"]()
                calls["float"]()
            device.synchronize()
        else:
            t = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k in calls:
                    t[k].append(per_launch_ms(calls[k]))
            copy_ms = float(np.median(t["copy"]))
            for k, wbytes in (("q8", qbytes), ("float", fbytes)):
                ms = float(np.median(t[k]))
                floor_ms = (in_bytes + wbytes) / 8e12 * 1e3
                rows.append({"shape": shape, "call": k, "read_MiB": in_bytes >> 20, "written_MiB": wbytes >> 20, "ms": round(ms, 4),
                             "spread": round(max(t[k]) / min(t[k]) - 1.0, 4), "floor_ms_at_8TBps": round(floor_ms, 4),
                             "frac_of_floor": round(floor_ms / ms, 3), "moved_TBps": round((in_bytes + wbytes) / (ms * 1e-3) / 1e12, 2),
                             "copy_of_the_input_ms": round(copy_ms, 4), "copy_TBps_read_plus_write": round(2 * in_bytes / (copy_ms * 1e-3) / 1e12, 2),
                             "Gpairs_per_s": round(ni * ns * N / (ms * 1e-3) / 1e9, 1)})
                print(json.dumps(rows[-1]), flush=True)
        for d in (d_in, d_f, d_q, d_taps, d_tw, d_g, d_n):
            d.free()
    print(json.dumps({"channeliser": rows}), flush=True)
    g.close()


def cmd_rfi(args):
    """The RFI flagger (include/dcs_rfi.h).  Per shape (beams x spectra x channels x block_len): the statistics pass, the flags
    and the cleaning (out of place, all three kinds of flags, with the counter) on noise-like bytes, beside stokes_block -- the
    project's read-bound streaming kernel -- over the same number of input bytes, in turn ``--rounds`` times in one process;
    then the dedispersion of the same spectra at ``--nr-dm`` DMs (the band of the dedisperse subcommand).  The hot calls and
    the yardstick rotate over two copies of their input, so that no call finds its bytes in the Infinity Cache.  Floors: the
    bytes a call must move at 8 TB/s -- B T C read by the statistics, read and written by the cleaning."""
    from dc_sand_amd.generator import (RfiThresholds, block_stokes_bytes, dm_delays_bytes, dm_time_bytes, filterbank_bytes,
                                       quantised_beams_bytes, rfi_cell_flags_bytes, rfi_cell_sums_bytes, rfi_channel_mask_bytes,
                                       rfi_counts_bytes, rfi_spectrum_flags_bytes, rfi_zero_dm_bytes)

    rows = []
    for text in args.shapes.split(","):
        B, T, C, n = (int(x) for x in text.lower().split("x"))
        nb, nr_dm = T // n, args.nr_dm
        assert nb * n == T and (B * T * C) % 65536 == 0
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
        g = SteeringCoefficientGenerator(bp)
        band, dms = (1500.0, -300.0 / C, 64e-6), np.linspace(0.0, 500.0, nr_dm)
        tb, pb = dm_delays_bytes(bp, nr_dm), dm_time_bytes(B, nr_dm, T)
        d_dms, d_delays, d_plane = device.mem_alloc(dms.nbytes), device.mem_alloc(tb), device.mem_alloc(pb)
        device.memcpy_htod(d_dms, dms)
        g.dm_delays(*band, d_dms, nr_dm, d_delays, tb)
        device.synchronize()
        table = np.empty((nr_dm, C), np.int32)
        device.memcpy_dtoh(table, d_delays)
        max_delay = int(table.max())
        in_spectra = T + max_delay
        fb = filterbank_bytes(bp, B, in_spectra)
        bufs = [device.mem_alloc(fb) for _ in range(2)]
        for d in bufs:
            _noise(d, fb)
        d_clean = device.mem_alloc(fb)
        sizes = (rfi_cell_sums_bytes(bp, B, nb), rfi_zero_dm_bytes(B, T), rfi_cell_flags_bytes(bp, B, nb), rfi_channel_mask_bytes(bp, B),
                 rfi_spectrum_flags_bytes(B, T), rfi_counts_bytes(B), 8 * B)
        d_cs, d_z, d_cf, d_cm, d_sf, d_cnt, d_rep = (device.mem_alloc(s) for s in sizes)
        device.memset(d_rep, 0, 8 * B)
        turn = [0]

        def buf():
            turn[0] ^= 1
            return bufs[turn[0]]
        moments = lambda: g.rfi_moments(buf(), fb, in_spectra, 0, nb, n, B, d_cs, sizes[0], d_z, sizes[1])  # noqa: E731
        moments_only = lambda: g.rfi_moments(buf(), fb, in_spectra, 0, nb, n, B, d_cs, sizes[0])  # noqa: E731
        flags = lambda: g.rfi_flags(d_cs, sizes[0], nb, n, B, d_cf, sizes[2], d_cm, sizes[3], d_cnt, sizes[5],  # noqa: E731
                                    thresholds=RfiThresholds(max_bad_blocks=2), d_zero_dm=d_z, zero_dm_bytes=sizes[1],
                                    d_spectrum_flags=d_sf, spectrum_flags_bytes=sizes[4])
        clean = lambda: g.rfi_clean_q8(buf(), fb, in_spectra, 0, nb, n, B, 128, d_clean, fb, in_spectra, d_cell_flags=d_cf,  # noqa: E731
                                       d_channel_mask=d_cm, d_spectrum_flags=d_sf, d_replaced=d_rep)
        dedisp = lambda: g.dedisperse_q8(bufs[0], fb, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_plane, pb, T)  # noqa: E731
        # the yardstick: 64 beams x 256 samples of two polarisations in Cs channels are B T C bytes
        Bs, nts, Cs = 64, 256, B * T * C // 65536
        bps = BeamformerParameters(NR_CHANNELS=Cs, NR_STATIONS=1, NR_BEAMS=Bs, NR_SAMPLES_PER_CHANNEL=nts)
        gs = SteeringCoefficientGenerator(bps)
        qb, sb1 = quantised_beams_bytes(bps, nts), block_stokes_bytes(bps, nts, 1)
        assert 2 * qb == B * T * C
        sbufs = [device.mem_alloc(2 * qb) for _ in range(2)]
        for d in sbufs:
            _noise(d, 2 * qb)
        d_bs = device.mem_alloc(sb1)

        def stokes():
            turn[0] ^= 1
            d = int(sbufs[turn[0]])
            gs.stokes_block(d, d + qb, qb, d_bs, sb1, nts, nr_stokes=1)
        for fn in (moments, moments_only, flags, clean, stokes):
            fn()
        device.synchronize()
        if args.trace:
            for fn in (moments, flags, clean, stokes) * 3:
                fn()
            device.synchronize()
            continue
        t = {name: [] for name in ("moments", "moments_only", "flags", "clean", "stokes", "dedisperse")}
        for _ in range(args.rounds):
            t["moments"].append(per_launch_ms(moments))
            t["stokes"].append(per_launch_ms(stokes))
            t["clean"].append(per_launch_ms(clean))
            t["stokes"].append(per_launch_ms(stokes))
            t["moments_only"].append(per_launch_ms(moments_only))
            t["flags"].append(per_launch_ms(flags))
        dedisp()
        device.synchronize()
        for _ in range(min(args.rounds, 3)):
            t["dedisperse"].append(per_launch_ms(dedisp, settle_ms=100.0, timed_ms=200.0))
        med = {name: float(np.median(x)) for name, x in t.items()}
        nbytes = B * T * C
        floor_us = nbytes / 8e12 * 1e6
        stage = med["moments"] + med["flags"] + med["clean"]
        row = {"shape": f"B={B} T={T} C={C} block_len={n}", "bytes_MiB": nbytes >> 20, "max_delay": max_delay, "nr_dm": nr_dm,
               "moments_us": round(med["moments"] * 1e3, 1), "moments_floor_us": round(floor_us, 1),
               "moments_share_of_floor": round(floor_us / (med["moments"] * 1e3), 3),
               "moments_without_zero_dm_us": round(med["moments_only"] * 1e3, 1),
               "clean_us": round(med["clean"] * 1e3, 1), "clean_floor_us": round(2 * floor_us, 1),
               "clean_share_of_floor": round(2 * floor_us / (med["clean"] * 1e3), 3),
               "flags_us": round(med["flags"] * 1e3, 1),
               "stokes_us": round(med["stokes"] * 1e3, 1), "stokes_spread": round(max(t["stokes"]) / min(t["stokes"]) - 1.0, 4),
               "moments_over_stokes": round(med["moments"] / med["stokes"], 3), "clean_over_stokes": round(med["clean"] / med["stokes"], 3),
               "spreads": {k: round(max(v) / min(v) - 1.0, 4) for k, v in t.items()},
               "rfi_stage_us": round(stage * 1e3, 1), "dedisperse_ms": round(med["dedisperse"], 3),
               "rfi_stage_over_dedisperse": round(stage / med["dedisperse"], 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        gs.close()
        for d in bufs + sbufs + [d_clean, d_dms, d_delays, d_plane, d_cs, d_z, d_cf, d_cm, d_sf, d_cnt, d_rep, d_bs]:
            d.free()
    print(json.dumps({"rfi": rows}), flush=True)


def cmd_fold(args):
    """The pulsar folder (include/dcs_fold.h).  Per (shape, nbin): fold_q8 with hits on noise-like bytes -- BEAMS beams, CHANNELS
    channels, SPECTRA spectra cut into sub-integrations of ``--subint-len``, each channel read at the delay of a DM of
    ``--dm`` -- beside fold_q8 without hits, fold_scrunch, and dedisperse_q8 with that one DM over the same window (existing code
    that reads the same bytes through the same gather), in turn ``--rounds`` times in one process.  The fold and the
    dedispersion rotate over two copies of the input, so that no call finds its bytes in the Infinity Cache.  Floor: the window
    read once plus the profiles written once at 8 TB/s."""
    from dc_sand_amd.fold import fold_models
    from dc_sand_amd.generator import (dm_delays_bytes, dm_time_bytes, filterbank_bytes, fold_hits_bytes, fold_profiles_bytes,
                                       fold_scrunched_bytes)

    rows = []
    for text in args.shapes.split(","):
        B, T, C = (int(x) for x in text.lower().split("x"))
        L = min(args.subint_len, T)
        S = T // L
        assert S * L == T
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
        g = SteeringCoefficientGenerator(bp)
        band, dms = (1500.0, -300.0 / C, 64e-6), np.full(B, args.dm, np.float64)
        tb = dm_delays_bytes(bp, B)
        d_dms, d_delays = device.mem_alloc(dms.nbytes), device.mem_alloc(tb)
        device.memcpy_htod(d_dms, dms)
        g.dm_delays(*band, d_dms, B, d_delays, tb)
        device.synchronize()
        table = np.empty((B, C), np.int32)
        device.memcpy_dtoh(table, d_delays)
        max_delay = int(table.max())
        in_spectra = T + max_delay
        fb = filterbank_bytes(bp, B, in_spectra)
        bufs = [device.mem_alloc(fb) for _ in range(2)]
        for d in bufs:
            _noise(d, fb)
        models = np.stack([fold_models(173.6879 + 0.01 * p, -1.7e-15, 0.125 * p, band[2], L, S) for p in range(B)])
        d_models = device.mem_alloc(models.nbytes)
        device.memcpy_htod(d_models, np.ascontiguousarray(models))
        pb1 = dm_time_bytes(B, 1, T)
        d_plane = device.mem_alloc(pb1)
        turn = [0]

        def buf():
            turn[0] ^= 1
            return bufs[turn[0]]
        dedisp = lambda: g.dedisperse_q8(buf(), fb, in_spectra, 0, T, B, d_delays, 1, max_delay, d_plane, pb1, T)  # noqa: E731
        for nbin in (int(x) for x in args.nbins.split(",")):
            pb, hb, sb = fold_profiles_bytes(bp, B, S, nbin), fold_hits_bytes(B, S, nbin), fold_scrunched_bytes(B, S, nbin)
            d_p, d_h, d_s = device.mem_alloc(pb), device.mem_alloc(hb), device.mem_alloc(sb)
            kw = dict(d_delays=d_delays, delays_bytes=tb, max_delay=max_delay)
            fold = lambda: g.fold_q8(buf(), fb, in_spectra, 0, L, S, B, d_models, models.nbytes, nbin, d_p, pb, S, d_hits=d_h,  # noqa: E731
                                     hits_bytes=hb, **kw)
            fold_only = lambda: g.fold_q8(buf(), fb, in_spectra, 0, L, S, B, d_models, models.nbytes, nbin, d_p, pb, S, **kw)  # noqa: E731
            scrunch = lambda: g.fold_scrunch(d_p, pb, B, S, 0, S, nbin, d_s, sb)  # noqa: E731
            for fn in (fold, fold_only, scrunch, dedisp):
                fn()
            device.synchronize()
            if args.trace:
                for fn in (fold, scrunch, dedisp) * 3:
                    fn()
                device.synchronize()
            else:
                t = {name: [] for name in ("fold", "fold_only", "scrunch", "dedisperse")}
                for _ in range(args.rounds):
                    t["fold"].append(per_launch_ms(fold))
                    t["dedisperse"].append(per_launch_ms(dedisp))
                    t["fold_only"].append(per_launch_ms(fold_only))
                    t["scrunch"].append(per_launch_ms(scrunch))
                med = {name: float(np.median(x)) for name, x in t.items()}
                floor_us = (B * in_spectra * C + pb) / 8e12 * 1e6
                row = {"shape": f"B={B} T={T} C={C} subint_len={L} nr_subints={S} nbin={nbin}", "max_delay": max_delay,
                       "window_MiB": (B * in_spectra * C) >> 20, "profiles_MiB": pb >> 20,
                       "fold_us": round(med["fold"] * 1e3, 1), "fold_without_hits_us": round(med["fold_only"] * 1e3, 1),
                       "floor_us": round(floor_us, 1), "fold_share_of_floor": round(floor_us / (med["fold"] * 1e3), 3),
                       "dedisperse_one_dm_us": round(med["dedisperse"] * 1e3, 1),
                       "fold_over_dedisperse": round(med["fold"] / med["dedisperse"], 3), "scrunch_us": round(med["scrunch"] * 1e3, 1),
                       "spreads": {k: round(max(v) / min(v) - 1.0, 4) for k, v in t.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
            for d in (d_p, d_h, d_s):
                d.free()
        g.close()
        for d in bufs + [d_dms, d_delays, d_models, d_plane]:
            d.free()
    print(json.dumps({"fold": rows}), flush=True)


def _spectra(d_x, C, B, T):
    """Realistic float spectra [T][C][B]: x = m_cb (1 + 0.25 g), m over 2^-20 .. 2^20 (eight seeded slices repeated)."""
    rng = np.random.default_rng(0xFB)
    m = np.exp2(rng.uniform(-20.0, 20.0, size=(C, B))).astype(np.float32)
    n = min(T, 8)
    device.memcpy_htod(d_x, (m[None] * (1.0 + 0.25 * rng.standard_normal((n, C, B), dtype=np.float32))).astype(np.float32))
    off, nbytes = n * C * B * 4, T * C * B * 4
    while off < nbytes:
        k = min(off, nbytes - off)
        device.memcpy_dtod(int(d_x) + off, d_x, k)
        off += k
    device.synchronize()


def cmd_fbank(args):
    """8-bit search filterbanks (include/dcs_filterbank.h).  The quantiser reads 4 bytes and writes 1 per element: 1.25 x
    the bytes of the read probe ``dcs_probe_reduce`` over the same input.  Per shape (T x C x B), in turn ``--rounds`` times
    in one process: the quantiser, the probe twice (its own spread; the probe call synchronises, allocates and copies 128 KiB
    back, so the kernel-to-kernel comparison is the one of ``--trace``), the sums call.  512 MiB of spectra exceed the
    Infinity Cache; the 256 MiB shape rotates over five buffers.  Then what sums + scales + quantiser add to the detecting
    call plus its integration at 64 antennas x 256 beams.  ``--trace``: five launches of each kernel and of the probe."""
    from dc_sand_amd.generator import (block_power_bytes, filterbank_bytes, filterbank_scales_bytes, power_spectra_bytes,
                                       spectra_sums_bytes)
    from probes import dcs_probes as pr

    rows = []
    for T, C, B, nbuf in [(128, 4096, 256, 1), (64, 4096, 256, 5)]:
        xb = T * C * B * 4
        d_xs = [device.mem_alloc(xb) for _ in range(nbuf)]
        for d in d_xs:
            _spectra(d, C, B, T)
        turn = [0]

        def d_x():
            turn[0] = (turn[0] + 1) % nbuf
            return d_xs[turn[0]]
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
        g = SteeringCoefficientGenerator(bp)
        nsums, nsc, nfb = spectra_sums_bytes(bp, B), filterbank_scales_bytes(bp, B), filterbank_bytes(bp, B, T)
        d_sums, d_sc, d_fb, d_clips = device.mem_alloc(nsums), device.mem_alloc(nsc), device.mem_alloc(nfb), device.mem_alloc(B * 8)
        device.memset(d_clips, 0, B * 8)
        sums = lambda: g.spectra_sums(d_x(), xb, T, B, d_sums, nsums)  # noqa: E731
        q8 = lambda: g.filterbank_q8(d_x(), xb, T, B, d_sc, 128.0, d_fb, nfb, T, descending=True, d_clip_count=d_clips)  # noqa: E731

        def probe_us():
            e0, e1 = device.Event(), device.Event()
            d = d_x()
            e0.record()
            pr.tensor_properties(d, xb)
            e1.record()
            e1.synchronize()
            return e1.elapsed_ms_since(e0)
        sums()
        g.filterbank_scales(d_sums, nsums, T, B, 24.0, d_sc, nsc)
        q8()
        probe_us()
        if args.trace:
            for _ in range(5):
                q8()
                sums()
                device.synchronize()
                pr.tensor_properties(d_x(), xb)
            print(f"trace {T}x{C}x{B}: {xb} bytes read per launch of each kernel, {nfb} written by the quantiser", flush=True)
        else:
            t = {name: [] for name in ("q8", "probe", "probe_again", "sums")}
            for _ in range(args.rounds):
                t["q8"].append(per_launch_ms(q8))
                t["probe"].append(float(np.median([probe_us() for _ in range(20)])))
                t["probe_again"].append(float(np.median([probe_us() for _ in range(20)])))
                t["sums"].append(per_launch_ms(sums))
            med = {name: float(np.median(x)) for name, x in t.items()}
            both = t["probe"] + t["probe_again"]
            spread = max(max(both) / min(both) - 1.0, abs(med["probe_again"] / med["probe"] - 1.0))
            row = {"shape": f"{T}x{C}x{B}", "input_MiB": xb >> 20, "buffers": nbuf,
                   "q8_us": round(med["q8"] * 1e3, 1), "q8_TBps": round((xb + nfb) / (med["q8"] * 1e-3) / 1e12, 2),
                   "probe_call_us": round(med["probe"] * 1e3, 1), "probe_call_again_us": round(med["probe_again"] * 1e3, 1),
                   "probe_call_TBps": round(xb / (med["probe"] * 1e-3) / 1e12, 2), "probe_spread": round(spread, 4),
                   "q8_over_probe_call": round(med["q8"] / med["probe"], 4),
                   "q8_within_condition": bool(med["q8"] <= med["probe"] * (1.25 + spread)),
                   "sums_us": round(med["sums"] * 1e3, 1), "sums_over_probe_call": round(med["sums"] / med["probe"], 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        g.close()
        for d in d_xs + [d_sums, d_sc, d_fb, d_clips]:
            d.free()
    if not args.trace:  # the pipeline: 64 antennas x 256 beams x 4096 channels, 1024 samples into 16 spectra of 4 blocks
        A, B, C, nt, n = 64, 256, 4096, 1024, 4
        nblk, T = nt // 16, nt // 16 // n
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        ab, pb, sb = A * C * nt * 2, block_power_bytes(bp, nt), power_spectra_bytes(bp, nblk, n)
        nsums, nsc, nfb = spectra_sums_bytes(bp, B), filterbank_scales_bytes(bp, B), filterbank_bytes(bp, B, T)
        bufs = [device.mem_alloc(x) for x in (ab, pb, sb, nsums, nsc, nfb)]
        d_ant, d_p, d_s, d_sums, d_sc, d_fb = bufs
        _noise(d_ant, ab)

        def detect():
            g.beamform_accumulated_power(d_ant, ab, d_p, pb, nt, t_coeff=1)
            g.integrate_block_power(d_p, pb, nblk, n, d_s, sb)

        def search():
            g.spectra_sums(d_s, sb, T, B, d_sums, nsums)
            g.filterbank_scales(d_sums, nsums, T, B, 24.0, d_sc, nsc)
            g.filterbank_q8(d_s, sb, T, B, d_sc, 128.0, d_fb, nfb, T, descending=True)
        detect()
        search()
        td = float(np.median([per_launch_ms(detect) for _ in range(args.rounds)]))
        ts = float(np.median([per_launch_ms(search) for _ in range(args.rounds)]))
        row = {"pipeline": f"{A}x{B}x{C}x{nt}, {T} spectra", "detect_and_integrate_us": round(td * 1e3, 1),
               "sums_scales_q8_us": round(ts * 1e3, 1), "added": round(ts / td, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
        for d in bufs:
            d.free()
        print(json.dumps({"fbank": rows}), flush=True)


def cmd_copy(args):
    """Mixed read + write ceiling: device-to-device copies (lean kernel in address order; hipMemcpyDtoD)."""
    from probes import dcs_probes as pr
    from dc_sand_amd import _lib

    nbytes = 4 * 2 ** 30
    a, b = device.mem_alloc(nbytes), device.mem_alloc(nbytes)
    device.memset(a, 1, nbytes)
    for per in (1, 2, 4, 8):
        for mode in (0, 1):
            ms = min(per_launch_ms(lambda: pr.copy(a, b, nbytes, mode, per), timed_ms=30) for _ in range(2))
            print(f"copy kernel, {per} x 16 B per thread, {'nontemporal' if mode else 'plain'} stores: {2 * nbytes / ms / 1e9:.2f} TB/s (read + write)", flush=True)
    ms = min(per_launch_ms(lambda: _lib.check(_lib.lib().dcs_memcpy_dtod(ctypes.c_void_p(int(b)), ctypes.c_void_p(int(a)), nbytes, None), "dtod"),
                           timed_ms=30) for _ in range(2))
    print(f"hipMemcpyDtoDAsync: {2 * nbytes / ms / 1e9:.2f} TB/s (read + write)", flush=True)


def cmd_mfma(args):
    """fp32 matrix-core issue rate on register operands (what the coefficient-reuse beamformer is measured against)."""
    from probes import dcs_probes as pr

    out = device.mem_alloc(1 << 20)
    for which, name, flop in ((0, "v_mfma_f32_16x16x4_f32, 2 accumulators", 2048), (1, "v_mfma_f32_16x16x4_f32, 4 accumulators", 2048),
                              (2, "v_mfma_f32_32x32x2_f32, 2 accumulators", 4096), (3, "16x16x4 with int8->fp32 conversions between", 2048),
                              (4, "16x16x4, A operands from LDS + conversions (the beamformer k-step)", 2048)):
        for blocks in (256, 512, 1024, 2048):
            iters = 4096
            ms = min(per_launch_ms(lambda: pr.mfma(which, blocks, iters, out), settle_ms=20, timed_ms=20) for _ in range(2))
            n = blocks * 4 * iters * (16 if which != 2 else 8)
            print(f"{name}, {blocks} workgroups ({blocks * 4 / 1024:.0f} waves per SIMD): {n * flop / ms / 1e9:.1f} TFLOP/s", flush=True)


TABLE_MODES = ("unchanged", "host", "device", "staged-host", "staged-host-pinned", "staged-device")


def stream_table_modes(args):
    """Per table mode: the period of a tick when EVERY tick brings a new table (two tables alternating), for the full
    tensor and a range of slabs.  host / device: the table comes with the tick (tick_dt(new_table) /
    tick_dt_from_global: copy or gather in front of the generator); staged-*: the table of tick k + 1 is staged right
    after tick k is enqueued (stage_table, pinned=True, stage_table_from_global) and the next tick consumes it."""
    from dc_sand_amd.parameters import delay_vals_dtype

    bp, g, _, full, buf = make(SHAPES["cfg3"], 32)
    stream = device.Stream()
    step_s = args.model_step_us * 1e-6
    tables = [simulate_input(bp), simulate_input(bp)]
    tables[1]["fPhase_rad"] += np.float32(0.25)
    pinned = []
    d_tables = []
    for t in tables:
        p = device.pagelocked_empty(bp.n_pairs, delay_vals_dtype)
        p[:] = t
        pinned.append(p)
        d = device.mem_alloc(t.nbytes)
        device.memcpy_htod(d, t)
        d_tables.append(d)
    g.autotune(buf, full, stream=stream)  # as bench.py: the full tensor, then the cadence slab (the other kernel variant)
    g.autotune(buf, min(full, 2560 * bp.n_pairs * 8), stream=stream)

    def tick_fn(st, mode):
        if mode == "unchanged":
            return lambda i: st.tick_dt(i * step_s)
        if mode == "host":
            return lambda i: st.tick_dt(i * step_s, tables[i % 2])
        if mode == "device":
            return lambda i: st.tick_dt_from_global(i * step_s, d_tables[i % 2])

        def staged(i):
            st.tick_dt(i * step_s)
            if mode == "staged-host":
                st.stage_table(tables[(i + 1) % 2])
            elif mode == "staged-host-pinned":
                st.stage_table(pinned[(i + 1) % 2], pinned=True)  # the two arrays never change: no reuse hazard
            else:
                st.stage_table_from_global(d_tables[(i + 1) % 2])
        return staged

    def period_us(fn, ticks, warm=20):
        for i in range(warm):
            fn(i)
        stream.synchronize()
        e0, e1 = device.Event(), device.Event()
        t0 = time.perf_counter()
        e0.record(stream)
        for i in range(ticks):
            fn(warm + i)
        e1.record(stream)
        e1.synchronize()
        return e1.elapsed_ms_since(e0) / ticks * 1e3, (time.perf_counter() - t0) / ticks * 1e6

    slabs = [int(x) for x in args.slabs.split(",")] if args.slabs else [2048, 2304, 2432, 2560, 2688, 2816, 3072]
    out = {"config": "64ant x 1024beam x 32768chan, fp32, one time step per tick, a new table on every tick (two alternating); "
                     f"model time advances {args.model_step_us} us per tick", "cadence_target_us": 200.0, "modes": {}}
    for mode in args.table_mode:
        res = {"slabs": []}
        for nc in ([] if args.skip_full else [bp.NR_CHANNELS]) + slabs:
            nbytes = nc * bp.n_pairs * 8
            g.upload_delays(tables[0], stream=stream)
            st = g.stream_begin(buf, nbytes, 0, nc, stream)
            dev_us, wall_us = period_us(tick_fn(st, mode), ticks=args.ticks if nc < bp.NR_CHANNELS else 60)
            st.end()
            r = dict(channels=nc, bytes=nbytes, period_us=dev_us, wall_us=wall_us, TBps=nbytes / dev_us / 1e6)
            if nc == bp.NR_CHANNELS:
                res["full_tensor"] = r
            else:
                res["slabs"].append(r)
            print(mode, json.dumps(r), flush=True)
        ok = [s for s in res["slabs"] if max(s["period_us"], s["wall_us"]) <= 200.0]
        res["largest_slab_at_200us"] = max(ok, key=lambda s: s["channels"]) if ok else None
        out["modes"][mode] = res
    print("SUMMARY", json.dumps(out), flush=True)
    g.close()


def cmd_stream(args):
    if args.table_mode:
        return stream_table_modes(args)
    bp, g, _, full, buf = make(SHAPES["cfg3"], 32)
    table = simulate_input(bp)
    stream = device.Stream()
    step_s = args.model_step_us * 1e-6

    def period_us(fn, ticks=200, warm=20):
        for i in range(warm):
            fn(i)
        stream.synchronize()
        e0, e1 = device.Event(), device.Event()
        t0 = time.perf_counter()
        e0.record(stream)
        for i in range(ticks):
            fn(warm + i)
        e1.record(stream)
        e1.synchronize()
        return e1.elapsed_ms_since(e0) / ticks * 1e3, (time.perf_counter() - t0) / ticks * 1e6

    out = {"config": "64ant x 1024beam x 32768chan, fp32, one time step per tick; model time advances "
                     f"{args.model_step_us} us per tick (dcs_bf_stream_tick_dt)", "cadence_target_us": 200.0, "slabs": []}

    def measure(nc, with_updates=False):
        nbytes = nc * bp.n_pairs * 8
        st = g.stream_begin(buf, nbytes, 0, nc, stream)
        if with_updates:
            dev_us, wall_us = period_us(lambda i: st.tick_dt(i * step_s, table if i % 16 == 0 else None), ticks=100, warm=10)
        else:
            dev_us, wall_us = period_us(lambda i: st.tick_dt(i * step_s))
        st.end()
        p_us, p_wall = period_us(lambda i: g.generate_slab_dt(buf, nbytes, 0, nc, [i * step_s], stream=stream))
        return dict(channels=nc, bytes=nbytes, graph_period_us=dev_us, graph_wall_us=wall_us, plain_period_us=p_us, plain_wall_us=p_wall,
                    graph_TBps=nbytes / dev_us / 1e6, plain_TBps=nbytes / p_us / 1e6)

    out["full_tensor"] = measure(bp.NR_CHANNELS)
    print("full tensor:", json.dumps(out["full_tensor"]), flush=True)
    for nc in (256, 512, 1024, 1536, 2048, 2304, 2560, 2816, 3072, 4096):
        r = measure(nc)
        out["slabs"].append(r)
        print(json.dumps(r), flush=True)
    ok = [s for s in out["slabs"] if max(s["graph_period_us"], s["graph_wall_us"]) <= 200.0]
    out["largest_slab_at_200us_graph"] = max(ok, key=lambda s: s["channels"]) if ok else None
    okp = [s for s in out["slabs"] if max(s["plain_period_us"], s["plain_wall_us"]) <= 200.0]
    out["largest_slab_at_200us_plain"] = max(okp, key=lambda s: s["channels"]) if okp else None
    out["with_table_update_every_16_ticks_2048ch"] = measure(2048, True)
    print("SUMMARY", json.dumps(out), flush=True)
    g.close()


def cmd_pmc(args):
    bp, g, _, nb, buf = make(SHAPES["cfg3"], 32)
    for _ in range(6):
        g.generate(buf, nb, t0=1, nt=1, bitwidth=1)
    for mode in (0, 4):
        g.set_tuning(math_mode=mode)
        for _ in range(6):
            g.generate(buf, g.output_bytes(0, 1), t0=1, nt=1, bitwidth=0)
    device.synchronize()
    g.close()
    A, B, C, nt = 64, 64, 4096, 64
    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(simulate_input(bp))
    d_ant = device.mem_alloc(A * C * nt * 2)
    device.memset(d_ant, 3, A * C * nt * 2)
    d_beams = device.mem_alloc(B * C * nt * 8)
    for _ in range(6):
        g.generate_and_beamform(d_ant, A * C * nt * 2, d_beams, B * C * nt * 8, 0, nt)
    device.synchronize()


def cmd_sustained(args):
    bp, g, bw, nb, buf = make(SHAPES["cfg3"], 32)
    n = bp.coeffs_per_time_step()
    if args.autotune:
        print("autotune:", g.autotune(buf, nb), flush=True)
    t_end = time.perf_counter() + args.seconds
    k = 0
    while time.perf_counter() < t_end:
        e0, e1 = device.Event(), device.Event()
        e0.record()
        for _ in range(100):
            g.generate(buf, nb, t0=1 + (k % 255), nt=1)
            k += 1
        e1.record()
        e1.synchronize()
        ms = e1.elapsed_ms_since(e0) / 100
        print(f"t={args.seconds - (t_end - time.perf_counter()):5.2f} s: {ms:.4f} ms -> {n / ms / 1e6:.1f} Gcoeff/s, {nb / ms / 1e9:.3f} TB/s", flush=True)
    g.close()


def cmd_stores(args):
    """Store-only probes (needs DCS_LIB_PATH=probes/libdcs_probes.so for --kind kernel)."""
    from probes import dcs_probes as pr

    nbytes = 16 * 2 ** 30
    buf = device.mem_alloc(nbytes)
    if args.kind == "pattern":  # rows x cols KiB matrix, workgroup rectangles of rb rows x qb KiB
        cols = args.cols_kib
        rows = nbytes // (cols * 1024)
        for qb in [int(v) for v in args.qb.split(",")]:
            for rb in [int(v) for v in args.rb.split(",")]:
                for mode in [int(v) for v in args.mode.split(",")]:
                    ms = per_launch_ms(lambda: pr.store_pattern(buf, rows, cols, qb, rb, args.order, args.xcd, mode, args.threads))
                    print(f"pattern qb={qb} rb={rb} order={args.order} xcd={args.xcd} mode={mode} threads={args.threads}: {nbytes / ms / 1e9:.2f} TB/s", flush=True)
    elif args.kind == "lean":  # no loop, no division: spt stores per thread, optional sleep before each
        for spt in [int(v) for v in args.spt.split(",")]:
            for pace in [int(v) for v in args.pace.split(",")]:
                for mode in [int(v) for v in args.mode.split(",")]:
                    ms = per_launch_ms(lambda: pr.one_store(buf, nbytes, mode | (pace << 8), spt, 512 * 1024))
                    print(f"lean stores/thread={spt} pace={pace} mode={mode}: {nbytes / ms / 1e9:.2f} TB/s", flush=True)
    else:  # the real kernel, with and without arithmetic, paced
        bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=64, NR_BEAMS=1024)
        g = SteeringCoefficientGenerator(bp)
        g.upload_delays(simulate_input(bp))
        for cpb in [int(v) for v in args.cpb.split(",")]:
            for pace in [int(v) for v in args.pace.split(",")]:
                for nomath in (False, True):
                    g.set_tuning(form=1, tiles_per_block=1, chan_per_block=cpb, nontemporal=1)
                    pr.set_knobs(g, pace=pace, nomath=int(nomath))  # include/dcs_probes.h (the probes build behind the wrappers)
                    ms = per_launch_ms(lambda: g.generate(buf, nbytes, t0=1, nt=1))
                    print(f"kernel cpb={cpb} pace={pace} nomath={int(nomath)}: {nbytes / ms / 1e9:.2f} TB/s", flush=True)
        g.close()
    ms = per_launch_ms(lambda: device.memset(buf, 0, nbytes))
    print(f"hipMemsetAsync: {nbytes / ms / 1e9:.2f} TB/s", flush=True)


def cmd_sincos(args):
    """Every fp32 in [1, 128) through the device sincos forms against (float)sin((double)x)."""
    from probes import dcs_probes as pr

    x = np.arange(0x3F800000, 0x43000000, dtype=np.uint32).view(np.float32)
    n = x.size
    dx, ds, dc = device.mem_alloc(4 * n), device.mem_alloc(4 * n), device.mem_alloc(4 * n)
    device.memcpy_htod(dx, x)
    es = np.sin(x.astype(np.float64)).astype(np.float32).view(np.int32).astype(np.int64)
    ec = np.cos(x.astype(np.float64)).astype(np.float32).view(np.int32).astype(np.int64)
    for which, name in ((0, "library fast path (full polynomials)"), (3, "library fast path (low degree)"), (1, "__ocml_sincos_f32"), (2, "fp64 slow path")):
        pr.sincos(which, dx, n, ds, dc)
        device.synchronize()
        s, c = np.empty(n, np.float32), np.empty(n, np.float32)
        device.memcpy_dtoh(s, ds)
        device.memcpy_dtoh(c, dc)
        us = np.abs(np.where(s.view(np.int32) < 0, -(s.view(np.int32).astype(np.int64) & 0x7FFFFFFF), s.view(np.int32).astype(np.int64)) - np.where(es < 0, -(es & 0x7FFFFFFF), es))
        uc = np.abs(np.where(c.view(np.int32) < 0, -(c.view(np.int32).astype(np.int64) & 0x7FFFFFFF), c.view(np.int32).astype(np.int64)) - np.where(ec < 0, -(ec & 0x7FFFFFFF), ec))
        print(f"{name}: sin max {us.max()} ULP ({int((us > 1).sum())} over 1), cos max {uc.max()} ULP ({int((uc > 1).sum())} over 1)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("geometry")
    p.add_argument("--shapes", default="cfg2,mid,cfg3,cfg4,narrow")
    p.add_argument("--bits", type=int, default=32, choices=[16, 32])
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--form", type=int, default=0, help="form of the sweep's explicit geometries (0 = library's choice, 1 / 3)")
    p.add_argument("--verbose", action="store_true")
    p = sub.add_parser("refshape")
    p.add_argument("--sweep", action="store_true")
    p = sub.add_parser("fp16")
    p.add_argument("--modes", default="0,4")
    p.add_argument("--cpb", default="64,128,256")
    p.add_argument("--wpc", default="-1")
    p.add_argument("--tpb", default="1")
    p.add_argument("--form", type=int, default=1, help="1 = per-workgroup terms, 3 = terms table, 0 = library's choice")
    p.add_argument("--bits", type=int, default=16, choices=[16, 32])
    sub.add_parser("fused")
    p = sub.add_parser("bfweights")
    p.add_argument("--rounds", type=int, default=5, help="alternations of unweighted and weighted timings per shape")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape only (counter passes)")
    p.add_argument("--kind", default="acc", choices=["acc", "fused"], help="with --shape: which beamformer")
    p = sub.add_parser("bfpower")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the float and the power timings per shape")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape, a few launches of one call (counter passes)")
    p.add_argument("--variant", default="power", choices=["float", "power", "power+int"],
                   help="with --shape: float call, detecting call, detecting call + integration")
    p = sub.add_parser("bfcomplex")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the element-wise and the complex timings per shape")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape only")
    p = sub.add_parser("bfcq8")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the complex float, the complex int8 and the int8 timings per shape")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape only")
    p = sub.add_parser("incoh")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the new call and the read probe per shape")
    p.add_argument("--trace", action="store_true", help="a few launches of the new kernel and the probe only (kernel trace)")
    p = sub.add_parser("stokes")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the IQUV call, the I call and the incoherent beam per shape")
    p = sub.add_parser("dedisperse")
    p.add_argument("--rounds", type=int, default=5, help="timings of each call")
    p.add_argument("--shape", default="4096x512x16384x4", help="CxDMSxTxB with the table dm_delays makes")
    p.add_argument("--direct-shape", default="4096x32x2048x1", help="CxDMSxTxB with a seeded random table")
    p = sub.add_parser("single_pulse")
    p.add_argument("--rounds", type=int, default=5, help="timings of each call")
    p.add_argument("--shape", default="4096x512x16384x4", help="CxDMSxTxB: the shape of dedisperse")
    p.add_argument("--block-len", type=int, default=256, help="spectra per block of the peak plane")
    p.add_argument("--buffers", type=int, default=3, help="copies of the planes the rotated timings walk")
    p = sub.add_parser("candidates")
    p.add_argument("--rounds", type=int, default=5, help="timings of each call")
    p.add_argument("--shape", default="4096x512x16384x4", help="CxDMSxTxB: the shape of dedisperse")
    p.add_argument("--block-len", type=int, default=64, help="spectra per block of the peak plane")
    p.add_argument("--threshold", type=float, default=6.0)
    p.add_argument("--dm-radius", type=int, default=8)
    p.add_argument("--block-radius", type=int, default=8)
    p.add_argument("--max-candidates", type=int, default=4096)
    p = sub.add_parser("correlator")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the correlator and the incoherent beam per shape")
    p.add_argument("--shapes", default="64x4096x4096x64,256x1024x4096x64", help="AxCxNTxN, comma-separated: n blocks per visibility")
    p.add_argument("--buffers", type=int, default=2, help="copies of the samples that the timings rotate over, at least")
    p = sub.add_parser("ddc")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the one-band and the two-band call")
    p.add_argument("--shape", default="128x16777216", help="INPUTSxSAMPLES: rows of int8 samples")
    p.add_argument("--trace", action="store_true", help="a few launches only (a counter run of its own)")
    p = sub.add_parser("channeliser")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the quantised call, the float call and the copy per shape")
    p.add_argument("--shapes", default="64x1024x8x8192,64x64x4x131072,64x2048x16x4096", help="INPUTSxNxPxSPECTRA, comma-separated")
    p.add_argument("--trace", action="store_true", help="a few launches only (a counter run of its own)")
    p = sub.add_parser("rfi")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the three calls and the Stokes yardstick per shape")
    p.add_argument("--shapes", default="4x16384x4096x256,4x16384x4100x256", help="BEAMSxSPECTRAxCHANNELSxBLOCK_LEN, comma-separated")
    p.add_argument("--nr-dm", type=int, default=512, help="DMs of the dedispersion that the stage is compared with")
    p.add_argument("--trace", action="store_true", help="a few launches only (a counter run of its own)")
    p = sub.add_parser("fold")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the fold, the one-DM dedispersion and the scrunch per shape and nbin")
    p.add_argument("--shapes", default="4x131072x4096", help="BEAMSxSPECTRAxCHANNELS, comma-separated")
    p.add_argument("--nbins", default="64,256,1024", help="phase bins, comma-separated")
    p.add_argument("--subint-len", type=int, default=8192, help="spectra of a sub-integration (it divides SPECTRA)")
    p.add_argument("--dm", type=float, default=100.0, help="the DM of the delay row of every beam")
    p.add_argument("--trace", action="store_true", help="a few launches only (a counter run of its own)")
    p = sub.add_parser("fbank")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the quantiser, the read probe and the sums per shape")
    p.add_argument("--trace", action="store_true", help="a few launches of the new kernels and the probe only (kernel trace)")
    p = sub.add_parser("bfq8")
    p.add_argument("--rounds", type=int, default=5, help="alternations of the float and the int8 timings per shape")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape, a few launches of one call (counter passes)")
    p.add_argument("--variant", default="q8", choices=["float", "q8", "q8c"], help="with --shape: float call, int8 call, int8 call with counters")
    sub.add_parser("mfma")
    sub.add_parser("copy")
    p = sub.add_parser("bfacc")
    p.add_argument("--shape", default="", help="AxBxCxNT: one shape only (PMC passes)")
    p.add_argument("--modes", default="0,8", help="math_mode values: 0 = int8 fixed point, 8 = fp32 chain")
    p.add_argument("--random", action="store_true", help="noise-like int8 samples instead of a constant byte (the matrix pipe's power depends on the data)")
    p = sub.add_parser("bfreplay")
    p.add_argument("--rounds", type=int, default=5, help="timings of each of the three ways; the last two alternate")
    p.add_argument("--shape", default="64x16x640x272", help="AxBxCxNT")
    p = sub.add_parser("stream")
    p.add_argument("--model-step-us", type=float, default=200.0)
    p.add_argument("--table-mode", action="append", choices=TABLE_MODES,
                   help="measure per way of bringing a new table to every tick (repeatable); without it: the round-3 report")
    p.add_argument("--slabs", default="", help="with --table-mode: comma-separated slab widths in channels")
    p.add_argument("--skip-full", action="store_true", help="with --table-mode: no full-tensor run")
    p.add_argument("--ticks", type=int, default=200, help="with --table-mode: timed ticks per slab")
    sub.add_parser("pmc")
    p = sub.add_parser("sustained")
    p.add_argument("--seconds", type=float, default=6.0)
    p.add_argument("--autotune", action="store_true")
    p = sub.add_parser("stores")
    p.add_argument("--kind", default="lean", choices=["pattern", "lean", "kernel"])
    p.add_argument("--qb", default="1")
    p.add_argument("--rb", default="4,8,16")
    p.add_argument("--order", type=int, default=0)
    p.add_argument("--xcd", type=int, default=0)
    p.add_argument("--mode", default="1")
    p.add_argument("--threads", type=int, default=256)
    p.add_argument("--cols-kib", type=int, default=512, help="row length of the pattern matrix in KiB (32: the beamformer's output at 256 beams)")
    p.add_argument("--spt", default="1,2,3,4,8")
    p.add_argument("--pace", default="0")
    p.add_argument("--cpb", default="8,12,16")
    sub.add_parser("sincos")
    args = ap.parse_args()
    device.require_device()
    device.set_device(0)
    print("device:", device.device_name(0), flush=True)
    {"geometry": cmd_geometry, "refshape": cmd_refshape, "fp16": cmd_fp16, "fused": cmd_fused, "bfweights": cmd_bfweights, "bfq8": cmd_bfq8, "bfpower": cmd_bfpower, "bfcomplex": cmd_bfcomplex, "bfcq8": cmd_bfcq8, "incoh": cmd_incoh, "stokes": cmd_stokes, "dedisperse": cmd_dedisperse, "single_pulse": cmd_single_pulse, "candidates": cmd_candidates, "correlator": cmd_correlator, "ddc": cmd_ddc, "channeliser": cmd_channeliser, "rfi": cmd_rfi, "fold": cmd_fold, "fbank": cmd_fbank, "mfma": cmd_mfma, "copy": cmd_copy, "bfacc": cmd_bfacc, "bfreplay": cmd_bfreplay, "stream": cmd_stream, "pmc": cmd_pmc,
     "sustained": cmd_sustained, "stores": cmd_stores, "sincos": cmd_sincos}[args.cmd](args)


if __name__ == "__main__":
    main()

"""Regenerates tests/golden/ddc/: the reference's CPU down-converter (feng/ddc/src/ddc.py with cwg.py, which need scipy) run
on int8 inputs, with the integers behind its two filter designs.  The reference tree is imported at generation time only:

    python tests/golden/make_ddc_golden.py --reference /path/to/reference/checkout

Cases (sampling 1712 MHz, mixing 100 MHz, the 107 MHz design, decimation 16):
  random     N = 4097 seeded full-range int8
  centre, dual, bandedge, outofband
             the four scenarios of feng/ddc/testing/test_ddc.py at N = 8193: cwg.py's tones at amplitude 60, summed and rounded
             to int8.
N - 1 is a power of two, so that cwg.py's oscillator step int(N f / f_s) / (N - 1) = 239 / 4096 turns per sample is exactly
the 32-bit phase step 239 * 2^20.

Each case is an .npz of x (int8 [N]) and y (complex128, ddc.py's output); taps.npz holds each design's decimals as the CSV
prints them (c107, c53) and their integers over 2^17 (h107, h53).  manifest.json lists the files with their SHA-256, the
parameters, and what this script measured: the largest |model - reference| per case against the smallest tolerance
(tests/helpers/ddc_model.py), and per scenario the reference's own tone bins and rejection in a 256-point spectrum of its last
256 outputs.  The filters are symmetric, so the reference's convolution order and the correlation order of the taps coincide;
the script checks that.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "ddc"
F_S, F_MIX, DECIMATION, SCALE_BITS, FFT = 1712e6, 100e6, 16, 5, 256
SCENARIOS = {  # name: tone frequencies (test_ddc.py)
    "centre": (100e6,),
    "dual": (100e6, 103343750.0),
    "bandedge": (51019287.109375, 148980712.890625),
    "outofband": (100e6, 214e6),
}
IN_BAND = {"centre": (100e6,), "dual": (100e6, 103343750.0), "bandedge": (51019287.109375, 148980712.890625), "outofband": (100e6,)}


def tone_bins(freqs):
    """test_ddc.py's expected channels: floor((f - f_mix) / (f_s / 16 / fft_length)), and below the mixing frequency
    fft_length - floor((f_mix - f) / (f_s / 16 / fft_length))."""
    width = F_S / DECIMATION / FFT
    return sorted(int(np.floor((f - F_MIX) / width)) if f >= F_MIX else FFT - int(np.floor((F_MIX - f) / width)) for f in freqs)


def rejection_db(y, bins):
    """The reference's figure: the weakest expected bin over the strongest other bin of fft(last 256 outputs)^2, in dB."""
    p = np.abs(np.fft.fft(y[-FFT:]) ** 2)
    others = np.delete(p, bins)
    return float(10.0 * np.log10(p[bins].min() / others.max())), sorted(int(b) for b in np.argsort(p)[-len(bins):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds feng/ddc/src/ddc.py)")
    args = ap.parse_args()
    src = Path(args.reference) / "feng" / "ddc" / "src"
    sys.path[:0] = [str(src), str(ROOT), str(ROOT / "tests")]
    import cwg  # noqa: E402  (the reference's)
    import ddc as ref_ddc  # noqa: E402  (the reference's)
    from dc_sand_amd import ddc as design  # noqa: E402
    from helpers import ddc_model as model  # noqa: E402

    OUT.mkdir(exist_ok=True)
    conv = {k: ref_ddc.DigitalDownConverter(DECIMATION, F_S, str(src / f"ddc_coeff_{k}MHz.csv")) for k in ("107", "53")}
    taps = {}
    for k, d in conv.items():
        c = np.asarray(d.ddc_filter_coeffs, dtype=np.float64)
        h = design.integer_taps(c)
        assert np.array_equal(h, h[::-1]) and np.array_equal(c, c[::-1]), "the design is not symmetric: reverse it for correlation order"
        taps["c" + k], taps["h" + k] = c, h.astype(np.int32)
    np.savez_compressed(OUT / "taps.npz", **taps)

    cases = {}
    N = 4097
    cases["random"] = np.random.default_rng(4097).integers(-128, 128, size=N, dtype=np.int8)
    N = 8193
    for name, freqs in SCENARIOS.items():
        tone = sum(cwg.generate_carrier_wave(cw_scale=1, freq=f, sampling_frequency=F_S, num_samples=N, noise_scale=0.0, complex=False)
                   for f in freqs)
        x = np.rint(60.0 * np.asarray(tone, dtype=np.float64))
        assert np.abs(x).max() <= 127
        cases[name] = x.astype(np.int8)

    manifest = {"generator": "tests/golden/make_ddc_golden.py", "sampling_frequency": F_S, "mixing_frequency": F_MIX,
                "decimation": DECIMATION, "design": "107", "scale_bits": SCALE_BITS, "fft_length": FFT, "files": {}, "cases": {}}
    h, c = taps["h107"], taps["c107"]
    for name, x in cases.items():
        N = x.size
        cycles = int(N / (F_S / F_MIX))
        step = design.phase_step(cycles, N - 1)  # cwg.py: linspace(0, cycles, N)
        assert step * (N - 1) == cycles << 32, "the oscillator step is no 32-bit phase step"
        y = np.asarray(conv["107"].run(x.astype(np.float64), F_MIX), dtype=np.complex128)
        np.savez_compressed(OUT / f"{name}.npz", x=x, y=y, phase_step=np.uint32(step))
        g, gain = design.band_taps(h, step, SCALE_BITS)
        got = model.as_complex(model.ddc(x[None, :], g[None], [(step, 0, gain)], y.size)[0, 0])
        tol = model.reference_tolerance(x, c, h, g, gain, SCALE_BITS, y)
        diff = np.abs(got - y)
        entry = {"N": int(N), "nr_out": int(y.size), "phase_step": int(step), "max_abs_y": float(np.abs(y).max()),
                 "max_abs_diff_model_vs_reference": float(diff.max()), "min_tolerance": float(tol.min()),
                 "max_diff_over_tolerance": float((diff / tol).max())}
        if name in SCENARIOS:
            bins = tone_bins(IN_BAND[name])
            db, top = rejection_db(y, bins)
            db_model, _ = rejection_db(got, bins)
            entry.update({"tone_bins": bins, "reference_top_bins": top, "reference_rejection_db": round(db, 2),
                          "reference_meets_60_db": bool(db >= 60.0 and top == bins), "model_rejection_db": round(db_model, 2)})
        manifest["cases"][name] = entry
        print(name, json.dumps(entry))
    for f in sorted(OUT.glob("*.npz")):
        manifest["files"][f.name] = {"bytes": f.stat().st_size, "sha256": hashlib.sha256(f.read_bytes()).hexdigest()}
    (OUT / "manifest.json").write_text(json.dumps(manifest, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()

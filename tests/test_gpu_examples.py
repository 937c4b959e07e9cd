"""What a user of the library runs first, on the GPU: the scripts under examples/, each in a fresh process, and the C++
host program written against the C-ABI (tests/cpp).  Each verifies its own output; parity with the CPU oracle test by test
is tests/test_gpu_parity.py."""
import pytest

pytestmark = pytest.mark.gpu

# What each script's closing line says once it has verified itself.  tied_array_beam.py ends with its table of beams, whose
# row of the source carries the mark; the two statistical scripts (a planted source that must stand out of the other beams)
# keep the antenna counts of their defaults, the bit-for-bit ones take ragged counts.
EXAMPLE_CLOSING = {
    "steering_coefficients.py": "max ULP distance to the CPU verifier",
    "streaming_ticks.py": "max ULP distance to the CPU verifier",
    "detected_beams.py": "bit-identical to the contract applied to the float call's beams: True",
    "incoherent_beam.py": "bit-identical to the integer contract: True",
    "search_filterbank.py": "bit-identical to the model: detected beams True - incoherent beam True",
    "tied_array_beam.py": "<- the source",
    "hierarchical_beams.py": "stage 2, mean |beam|: beam 0:",
    "dual_pol_stokes.py": "bit-identical to the integer contract: True",
}


@pytest.mark.parametrize("script,args", [("steering_coefficients.py", ["16", "24", "512"]), ("streaming_ticks.py", ["16", "64", "2048", "256", "20"]),
                                         ("detected_beams.py", ["20", "5", "6"]), ("incoherent_beam.py", ["20", "5", "6"]),
                                         ("search_filterbank.py", ["20", "5", "6"]), ("tied_array_beam.py", ["64", "16", "2"]),
                                         ("hierarchical_beams.py", ["64", "8", "2"]), ("dual_pol_stokes.py", ["20", "5", "6"])])
def test_examples_run_and_verify_themselves(gpu, script, args):
    """examples/: all eight scripts on small shapes, a fresh process each; each verifies its own output (against the oracle,
    a model, or the source it planted), says so in its closing line and exits 0."""
    from helpers.examples import run_example

    out = run_example(script, *args)
    assert EXAMPLE_CLOSING[script] in out, out[-1500:]


def test_cpp_host_against_c_abi(gpu):
    """The reference's harness is C++: tests/cpp/run_beamformer_tests.cpp is the
    runBeamformerTests executable written against the C-ABI (plain g++, no hipcc
    on the host side), with the C oracle as verify_output's expected data."""
    import subprocess
    from pathlib import Path

    d = Path(__file__).resolve().parent / "cpp"
    res = subprocess.run(["make", "-C", str(d)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(d / "run_beamformer_tests")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("CPU took") == 3
    for name in ("Combined Steering Coeffs+Beamforming", "Multiple Chans+Timestamps", "Multiple Channels", "Naive Implementation"):
        assert name in run.stdout

"""The examples as the tests run them: each in a fresh child process, which must end with status 0."""
import subprocess
import sys
from pathlib import Path

EXAMPLES = Path(__file__).resolve().parent.parent.parent / "examples"


def run_example(script, *args, timeout=600):
    """Runs examples/<script> with ``args`` and returns its stdout; what the output must say is the test's to assert."""
    res = subprocess.run([sys.executable, str(EXAMPLES / script), *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    return res.stdout

"""The run loop shared by the four plans (csrc/loop.h) against its specification, on the host alone."""
import os
import subprocess

from simrank_amd import _lib


def test_run_loop_against_its_specification_under_the_sanitizers():
    """make loop_check: tools/host/loop_check.cpp drives loop.h with a scripted fake over every combination of
    iterations 0..5, eps {0.5, 1, 1.5, NaN}, first zero count at update 1..5 or never, callback {null, never stopping,
    stopping at index 0..5}, speculation on / off and a failing queue / count call, under AddressSanitizer + UBSan, and
    compares updates_done, converged_at, the callback sequence, the returned code and the current update with the
    reference's loop written out plainly; the fake asserts the order of the calls.  No GPU needed."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "csrc")
    out = subprocess.run(["make", "-C", csrc, "loop_check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "cases passed" in out.stdout

#!/usr/bin/env python3
"""tests/golden/make_golden_ref_bank_ends.py — the reference's answers to the calls of tests/test_bank_ends_cpu.py, FROM THE REFERENCE
BUILD (oracle/_ref/libmeters_ref.so), in the manner of make_golden_ref_calls.py.

Runs that file's ref test against the live reference objects with MTR_RECORD_REF=1 and writes tests/golden/golden_ref_bank_ends_v1.npz:
for every call the test makes of the reference (the method, its scalar arguments and the sha1 of its input arrays), what it returned.
Where oracle/_ref cannot be built the test replays these answers; where it can, every live answer is held against them.  Rerun after
changing the test's inputs (tests/_bank_ends.py: S, N, P, ENDS).  Data only — no reference text."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from _oracle import build_ref, have_reference  # noqa: E402

if __name__ == "__main__":
    if not have_reference():
        build_ref()
    if not have_reference():
        sys.exit("oracle/_ref is not built: the reference's sources are needed to record its answers")
    env = dict(os.environ, MTR_RECORD_REF="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "ref",
                              "tests/test_bank_ends_cpu.py"], cwd=ROOT, env=env))

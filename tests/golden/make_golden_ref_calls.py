#!/usr/bin/env python3
"""tests/golden/make_golden_ref_calls.py — the reference's answers to the ref tests' own calls, FROM THE REFERENCE BUILD
(oracle/_ref/libmeters_ref.so).

Runs tests/test_oracle_vs_ref.py and tests/test_needle_oracle_vs_ref.py against the live reference objects with
MTR_RECORD_REF=1 and writes tests/golden/golden_ref_calls_v1.npz: for every call those tests make of the reference (the
method, its scalar arguments and the sha1 of its input arrays), what it returned.  Where oracle/_ref cannot be built, the
same tests replay these answers (tests/_oracle.py: RecordedReference); where it can, every live answer is held against
them.  Rerun after changing a ref test's inputs.  Data only — no reference text."""
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
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider",
                              "tests/test_oracle_vs_ref.py", "tests/test_needle_oracle_vs_ref.py"], cwd=ROOT, env=env))

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "ref: against the reference's own objects: oracle/_ref where it is built, their recorded answers elsewhere")


@pytest.fixture(scope="session")
def oracle():
    from _oracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def reference():
    """The reference's objects (oracle/_ref), each answer also held against its recording in tests/golden/ — or, where
    oracle/_ref cannot be built, that recording replayed.  MTR_RECORD_REF=1 (tests/golden/make_golden_ref_calls.py): the
    live objects, their answers written into a new recording at the end of the session."""
    from _oracle import CheckedReference, RecordedReference, Reference, build_ref, have_reference
    if not have_reference():
        try:
            build_ref()
        except Exception:
            pass
    if not have_reference():
        yield RecordedReference()
        return
    record = os.environ.get("MTR_RECORD_REF") == "1"
    ref = CheckedReference(Reference(), check=not record, record=record)
    yield ref
    if record:
        print("\nrecorded %d answers of the reference" % ref.save())

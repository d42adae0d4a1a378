"""Track lengths for the 30-band bank (include/mtr_ends.h) without a GPU: the surface, the oracle restatement that the GPU tests'
helper compares the engine with, and its per-stream point counts.  What the entry points compute is held on the GPU
(tests/test_gpu_bank_ends.py)."""
import os
import re

import numpy as np
import pytest

import _bank as B
import _bank_ends as E
import _bank_series as BS
import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference's answers to test_the_restatement_is_the_reference's calls (tests/golden/make_golden_ref_bank_ends.py)
REF_ENDS = os.path.join(HERE, "golden", "golden_ref_bank_ends_v1.npz")
NEW = ["mtr_engine_process_device_ends", "mtr_engine_process_host_ends", "mtr_engine_spectr_points"]
ERR_ARG = -1


def test_the_header_declares_the_three_entry_points_and_the_library_exports_them():
    assert M.exported_symbols("mtr_ends.h") == NEW
    assert not set(NEW) & set(M.exported_symbols()) and not set(NEW) & set(M.exported_symbols("mtr_spectr.h")) and not set(NEW) & set(M.exported_symbols("mtr_ragged.h"))
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_ends\.h"$', hdr, re.M)
    assert hdr.index('#include "mtr_ragged.h"') < hdr.index('#include "mtr_ends.h"') < hdr.index("mtr_engine_stream_frames (")
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    for n in ("process_device_ends", "process_ends", "spectr_points"):
        assert callable(getattr(M.Engine, n))


def test_a_null_argument_is_an_argument_error():
    f = np.zeros(1, np.uint64)
    assert M.lib.mtr_engine_process_device_ends(None, None, 0, 0, f.ctypes.data, None) == ERR_ARG
    assert M.lib.mtr_engine_process_host_ends(None, None, 0, 0, f.ctypes.data) == ERR_ARG
    assert M.lib.mtr_engine_spectr_points(None, 0, 0, f.ctypes.data) == ERR_ARG
    assert M.lib.mtr_last_error()


def test_the_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    """five streams: waves {0, 1, 2}, {2, 3, 4}, {4}; the ends between them are the stated set; one wave holds three different ends, one
    an end of 0 beside an open stream, one only streams that end early"""
    waves = [sorted({p // B.NBANDS for p in range(w * 64, min((w + 1) * 64, E.S * B.NBANDS))}) for w in range((E.S * B.NBANDS + 63) // 64)]
    assert waves == [[0, 1, 2], [2, 3, 4], [4]] and E.S * B.NBANDS % 64
    assert E.N // 128 == 4 and E.N % 128
    assert sorted({v for ends in E.ENDS.values() for v in ends}) == [0, 1, 2, 99, 100, 101, 127, 128, 129, 256, 257, 599, 600]
    per_wave = [[ends[s] for s in w] for ends in E.ENDS.values() for w in waves]
    assert any(len(set(v)) == 3 for v in per_wave)
    assert any(0 in v and E.N in v for v in per_wave)
    assert any(len(v) > 1 and all(0 < f < E.N for f in v) for v in per_wave)


@pytest.mark.parametrize("fill", [0, 50])
def test_the_helpers_point_counts_are_mtr_series_cut(fill):
    vals = sorted({v for ends in E.ENDS.values() for v in ends} | {50, 51, 349, 350})
    for period in (0, 1, E.P, 128, 1000):
        if fill >= period > 0:
            continue
        for n in (350, E.N):
            for f in vals:
                if f > n or (period == 0 and fill):
                    continue
                assert E.expected_points(fill, period, n, f) == M.series_cut(fill, period, n, f), (fill, period, n, f)
                # ... and the spectrum_runs the yardsticks make are that many (a stream that stays open ends no truncated block)
                if period and 0 < f < n:
                    assert len(E.cuts_of(fill + f, period)) == sum(E.expected_points(fill, period, n, f)), (fill, period, n, f)


@pytest.fixture(scope="module")
def ends_reference():
    """tests/conftest.py's `reference` on a recording of this file's own: the reference's objects (oracle/_ref, built here if it can be),
    each answer also held against its recording in REF_ENDS — or, where oracle/_ref cannot be built, that recording replayed; a call that
    is not recorded is a KeyError, never a comparison left out.  MTR_RECORD_REF=1: the live objects, their answers written to REF_ENDS."""
    from _oracle import CheckedReference, RecordedReference, Reference, build_ref, have_reference
    if not have_reference():
        try:
            build_ref()
        except Exception:
            pass
    if not have_reference():
        yield RecordedReference(REF_ENDS)
        return
    record = os.environ.get("MTR_RECORD_REF") == "1"
    ref = CheckedReference(Reference(), check=False, record=record)
    if not record:
        ref.recorded = RecordedReference(REF_ENDS)
    yield ref
    if record:
        print("\nrecorded %d answers of the reference" % ref.save(REF_ENDS))


@pytest.mark.ref
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_the_restatement_is_the_reference(oracle, ends_reference, mono):
    """Blocks of P plus a truncated block through the oracle's handle (tests/_bank_ends.oracle_cuts at the default speed) are, bit for
    bit, the reference's own code over the stream's own frames in blocks of P with the last one truncated (ref_batch_spectr, live or
    its recorded answers) — and the oracle's batch entry, which walks the frames the same way."""
    ref = ends_reference
    for s in range(E.S):
        x = B.stream_input(s, E.N)
        if mono:
            x = np.ascontiguousarray(np.stack([x[:, 0], x[:, 0]], 1))
        for f in sorted({ends[s] for ends in E.ENDS.values()} - {0}):
            ser, fin = E.oracle_cuts(oracle, x, E.cuts_of(f, E.P), speed=None, mono=mono)
            assert len(ser["val"]) == f // E.P + (1 if f % E.P else 0)
            assert BS.same(fin, oracle.spectr(x[:f], E.FS, E.P)), (s, f)
            assert BS.same(fin, ref.spectr(np.ascontiguousarray(x[:f]), E.FS, E.P)), (s, f, "the reference")

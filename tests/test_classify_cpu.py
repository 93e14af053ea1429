"""ksp_classify_cpu, the host loop of classify (csrc/classify_cpu.cpp), against the restatement of the definition
(tests/classify_restate.py) on the inputs of tests/classify_inputs.py, and the argument errors of the classify calls.  No GPU."""
import ctypes

import numpy as np
import pytest

import classify_inputs as CI
import classify_restate as CR
import sketch_inputs as I
from kspider_amd import engine

FULL = CI.FULL


same = CI.check_result


@pytest.mark.parametrize("k", [1, 21, 31, 32, 33, 64])
def test_equals_the_restatement(k):
    for key in CI.small_keys(k) + CI.edge_keys(k):
        case, kept, refs, (ref_keys, ref_off) = CI.restated(key, k)
        st = same(engine.classify_cpu(case.seq, case.offsets, k, ref_keys, ref_off, max_hash=FULL), CR.from_kept(kept, refs), (key, k))
        assert st["bases"] == sum(chr(b) in "ACGTacgt" for b in case.seq) and st["batches"] == 1
        assert st["table_keys"] == len(set().union(*map(set, refs))) and st["table_holders"] == sum(len(q) for q in refs)


def test_many_short_records_and_the_cut():
    case, kept, refs, (ref_keys, ref_off) = CI.restated(("reads", 0), 21)
    whole = CR.from_kept(kept, refs)
    same(engine.classify_cpu(case.seq, case.offsets, 21, ref_keys, ref_off, max_hash=FULL), whole, "reads")
    m = CI.middle_hits(whole["rows"])
    for min_hits in (m - 1, m, m + 1):
        same(engine.classify_cpu(case.seq, case.offsets, 21, ref_keys, ref_off, min_hits=min_hits, max_hash=FULL), CR.from_kept(kept, refs, min_hits), min_hits)


def test_threshold_is_inclusive_and_cuts_the_references_too():
    k = 21
    case, kept, refs, (ref_keys, ref_off) = CI.restated(("repeats", 0), k)
    hashes = sorted({h for run in kept for h in run})
    m = hashes[len(hashes) // 2]
    for max_hash in (m, m - 1, 0):
        cut = [[h for h in run if h <= max_hash] for run in kept]
        st = same(engine.classify_cpu(case.seq, case.offsets, k, ref_keys, ref_off, max_hash=max_hash), CR.from_kept(cut, refs), max_hash)
        assert st["table_keys"] == len({h for q in refs for h in q if h <= max_hash})   # reference hashes above max_hash are not in the table
    at = CR.from_kept([[h for h in run if h <= m] for run in kept], refs)
    below = CR.from_kept([[h for h in run if h <= m - 1] for run in kept], refs)
    assert sum(at["kept_windows"]) > sum(below["kept_windows"])


def test_no_reference_at_all_and_no_window():
    case = I.mixed()
    rows, arrays, _ = engine.classify_cpu(case.seq, case.offsets, 21, np.zeros(0, np.uint64), [0], max_hash=FULL)
    assert rows.size == 0 and not arrays["matched"].any() and (arrays["best_ref"] == engine.CLASSIFY_NO_REF).all() and arrays["kept_windows"].sum() > 0
    rows, arrays, st = engine.classify_cpu(b"NNNN\n", [0, 5], 3, [5, 6], [0, 2], max_hash=FULL)
    assert rows.size == 0 and st["valid_kmers"] == 0 and arrays["kept_windows"].tolist() == [0]


def _refuse(call, *args, code=engine.KSP_E_ARG, **kwargs):
    with pytest.raises(engine.KspError) as ei:
        call(*args, **kwargs)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def test_argument_errors():
    case, _, _, (ref_keys, ref_off) = CI.restated(("repeats", 0), 21)
    for bad_k in (0, 65, -3):
        _refuse(engine.classify_cpu, case.seq, case.offsets, bad_k, ref_keys, ref_off, max_hash=FULL)
    n = len(case.seq)
    for bad in ([0, 50, 40, n], [1, 40, n], [0, 40, n - 1], [0]):
        _refuse(engine.classify_cpu, case.seq, bad, 21, ref_keys, ref_off, max_hash=FULL)
    assert "min_hits" in _refuse(engine.classify_cpu, case.seq, case.offsets, 21, ref_keys, ref_off, min_hits=0, max_hash=FULL)
    assert "strictly ascending" in _refuse(engine.classify_cpu, case.seq, case.offsets, 21, [1, 5, 5, 9], [0, 1, 4], max_hash=FULL)
    assert "reference 1" in _refuse(engine.classify_cpu, case.seq, case.offsets, 21, [7, 9, 8], [0, 1, 3], max_hash=FULL)
    _refuse(engine.classify_cpu, case.seq, case.offsets, 21, [1, 2, 3], [1, 3], max_hash=FULL)
    _refuse(engine.classify_cpu, case.seq, case.offsets, 21, [1, 2, 3], [0, 3, 2], max_hash=FULL)
    _refuse(engine.classify_cpu, case.seq, case.offsets, 21, None, [0, 3], max_hash=FULL)      # NULL keys with entries
    _refuse(engine.classify_cpu, case.seq, case.offsets, 21, [1, 2, 3], None, max_hash=FULL)   # NULL offsets
    # a run ascends inside its reference only: the next may start below
    rows, _, _ = engine.classify_cpu(case.seq, case.offsets, 21, [8, 9, 1, 2], [0, 2, 4], max_hash=FULL)
    assert rows.size == 0


def test_null_result_pointers_are_refused():
    lib = engine.lib()
    seq = np.frombuffer(b"ACGTACGT\n", dtype=np.uint8)
    off, ref_keys, ref_off = np.array([0, 9], np.uint64), np.array([1], np.uint64), np.array([0, 1], np.uint64)
    a = np.zeros(1, np.uint32)
    out, nr = ctypes.c_void_p(), ctypes.c_uint64(0)
    arrays = [a.ctypes.data] * 6
    for hole in range(6):
        holed = list(arrays)
        holed[hole] = None
        assert lib.ksp_classify_cpu(seq.ctypes.data, 9, off.ctypes.data, 1, 4, FULL, 42, ref_keys.ctypes.data, ref_off.ctypes.data, 1, 1, ctypes.byref(out), ctypes.byref(nr),
                                    *holed, None) == engine.KSP_E_ARG
    assert lib.ksp_classify_cpu(seq.ctypes.data, 9, off.ctypes.data, 1, 4, FULL, 42, ref_keys.ctypes.data, ref_off.ctypes.data, 1, 1, None, ctypes.byref(nr), *arrays,
                                None) == engine.KSP_E_ARG
    assert lib.ksp_classify_cpu(seq.ctypes.data, 9, off.ctypes.data, 1, 4, FULL, 42, ref_keys.ctypes.data, ref_off.ctypes.data, 1, 1, ctypes.byref(out), ctypes.byref(nr),
                                *arrays, None) == engine.KSP_OK   # stats may be NULL
    lib.ksp_free(out)

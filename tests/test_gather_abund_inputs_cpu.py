"""The weighted gather restatement (tests/gather_abund_restate.py) against rows written out by hand, the builders of
tests/gather_abund_inputs.py against what they are named for, and the mirror of the weighted row.  No GPU."""
import ctypes
import math
import re
import statistics
from pathlib import Path

import numpy as np

import gather_abund_inputs as I
import gather_abund_restate as WR
import gather_restate
from kspider_amd import engine

TOP32 = I.TOP32

BY_HAND = {
    # (query, rank, source, overlap, unique, remaining, w_unique, w_found, sq, median2)
    "two_rounds": [(0, 1, 0, 3, 3, 3, 15, 15, 107, 10), (0, 2, 1, 2, 2, 1, 10, 25, 68, 10)],
    "partly_dead_segment": [(0, 1, 0, 4, 4, 3, 2002, 2002, 2000002, 1001), (0, 2, 1, 4, 2, 1, 10, 2012, 52, 10)],
    "same_hash_two_queries": [(0, 1, 0, 2, 2, 0, 8, 8, 34, 8), (1, 1, 0, 2, 2, 0, 70, 70, 4900, 70)],
    "zeros": [(0, 1, 0, 3, 3, 0, 4, 4, 16, 0)],
    "upper_word": [(0, 1, 0, 2, 2, 1, 8589934590, 8589934590, 2**65 - 2**34 + 2, 8589934590)],
    "max_matches_1": [(0, 1, 0, 3, 3, 2, 6, 6, 14, 4)],
}


def test_restatement_against_rows_written_out_by_hand():
    cases = I.hand_made_cases()
    assert set(cases) == set(BY_HAND)
    for name, case in cases.items():
        assert WR.gather(*case) == BY_HAND[name], name
    assert WR.split_sq(2**65 - 2**34 + 2) == (2**64 - 2**34 + 2, 1)


def test_first_six_fields_are_the_unweighted_rows():
    for case in list(I.hand_made_cases().values()) + [I.sizes_case(), I.digit_case(1), I.digit_case(40), I.equal_case(), I.dead_part_case(), I.tiles_case()]:
        db, q, a, m, k = case
        assert [r[:6] for r in WR.gather(db, q, a, m, k)] == gather_restate.gather(db, q, m, k)


def test_statistics_against_the_library_of_python():
    """median2 / 2 is statistics.median, and the spread is the population standard deviation"""
    for case in (I.sizes_case(), I.dead_part_case(), I.tiles_case()):
        db, q, a, m, k = case
        sets = [set(r) for r in db]
        for row in WR.gather(db, q, a, m, k):
            W = sum(a[row[0]])
            cols = WR.columns(row, W)
            assert cols[1] == row[6] / row[4] and cols[2] == row[9] / 2
            assert 0 <= cols[0] <= 1
        # the first row of a query takes its whole overlap: the values are those of S & Q
        first = [r for r in WR.gather(db, q, a, m, k) if r[1] == 1]
        for row in first:
            ab = dict(zip((int(x) for x in q[row[0]]), a[row[0]]))
            vals = [ab[h] for h in sets[row[2]] if h in ab]
            assert row[9] == 2 * statistics.median(vals) and row[6] == sum(vals)
            assert math.isclose(WR.columns(row, 1)[3], statistics.pstdev(vals), rel_tol=1e-9, abs_tol=1e-9)


def test_builders_make_what_they_are_named_for():
    db, q, a, m, k = I.sizes_case()
    rows = WR.gather(db, q, a, m, k)
    assert sorted(r[4] for r in rows) == sorted(I.TAKEN_SIZES) and all(r[3] == r[4] for r in rows)
    even = [r for r in rows if r[4] % 2 == 0]
    assert even
    for r in even:   # the two middle values differ: 3i and 3(i + 1)
        assert r[9] % 6 == 3
    for n_side in (1, 40):
        db, q, a, m, k = I.digit_case(n_side)
        rows = WR.gather(db, q, a, m, k)
        assert sorted(r[9] for r in rows) == sorted(lo + hi for lo, hi in I.DIGIT_EDGES)
        assert all((r[4] <= 64) == (n_side == 1) for r in rows)
    rows = WR.gather(*I.equal_case())
    assert [(r[4], r[9]) for r in rows] == [(100, 14), (10, 2 * TOP32), (3, 0)]
    assert rows[1][8] == 10 * TOP32 * TOP32 and WR.split_sq(rows[1][8])[1] > 0
    assert WR.columns(rows[0], 1)[3] == 0.0
    rows = WR.gather(*I.dead_part_case())
    assert [(r[2], r[3], r[4]) for r in rows] == [(0, 200, 200), (2, 150, 70), (1, 90, 50)]
    assert rows[2][6] == sum(range(1, 51)) and rows[2][9] == 25 + 26          # its own 50 alone
    assert rows[1][6] == 5 * sum(range(70)) and rows[1][9] == 5 * (34 + 35)
    db, q, a, m, k = I.tiles_case()
    shared = set(int(x) for x in q[0]) & set(int(x) for x in q[1])
    assert shared and any(a[0][list(q[0]).index(h)] != a[1][list(q[1]).index(h)] for h in shared)
    assert any(0 in run for run in a) and len({r[0] for r in WR.gather(db, q, a, m, k)}) == len(q)
    for row in WR.gather(*I.ones(I.tiles_case())):
        assert row[6] == row[4] == row[8] and row[9] == 2


def test_arrays():
    dk, do, qk, qa, qo = I.arrays(*I.hand_made_cases()["same_hash_two_queries"][:3])
    assert dk.tolist() == [10, 20] and do.tolist() == [0, 2] and qk.tolist() == [10, 20, 10, 20] and qa.tolist() == [3, 5, 70, 0] and qo.tolist() == [0, 2, 4]
    assert qa.dtype == np.uint32 and qk.dtype == np.uint64


def test_the_weighted_row_is_64_bytes_and_mirrored():
    names = ("query", "rank", "source", "overlap", "unique", "remaining", "w_unique", "w_found", "sq_lo", "sq_hi", "median2")
    assert ctypes.sizeof(engine.GatherWRow) == 64 and tuple(n for n, _ in engine.GatherWRow._fields_) == names
    assert engine.GATHER_WROW_DTYPE.itemsize == 64 and engine.GATHER_WROW_DTYPE.names == names
    assert [engine.GATHER_WROW_DTYPE.fields[n][1] for n in names] == [getattr(engine.GatherWRow, n).offset for n in names]
    text = (Path(__file__).resolve().parent.parent / "include" / "kspider_amd.h").read_text()
    body = re.search(r"typedef struct ksp_gather_wrow \{(.*?)\} ksp_gather_wrow;", text, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == list(names)
    for name in ("ksp_gather_abund_device", "ksp_gather_abund_host", "kspider_gather_abund", "ksp_sketch_cpu_abund", "ksp_sketch_device_abund",
                 "ksp_sketch_host_abund", "ksp_sig_read"):
        assert name in engine.ABI_SYMBOLS and hasattr(engine.lib(), name)
    assert engine.SKETCH_ABUND == 4 and re.search(r"#define KSP_SKETCH_ABUND 4ull", text)


def test_refusals_before_a_device_is_chosen():
    """NULL pointers, min_hashes 0 and bad offsets are KSP_E_ARG without a GPU"""
    import pytest
    dk, do, qk, qa, qo = I.arrays(*I.hand_made_cases()["two_rounds"][:3])
    for args in ((dk, do, qk, None, qo), (None, do, qk, qa, qo), (dk, do, None, qa, qo), (dk, None, qk, qa, qo)):
        with pytest.raises(engine.KspError) as ei:
            engine.gather_abund_host(*args)
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.gather_abund_host(dk, do, qk, qa, qo, min_hashes=0)
    assert ei.value.code == engine.KSP_E_ARG and "min_hashes" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_abund_host(dk, do, qk, qa, [1, 6])
    assert ei.value.code == engine.KSP_E_ARG

"""The gather tests' inputs and their restatement, checked without a GPU: the hand-made cases against rows written out by hand
(so that tests/gather_restate.py is pinned by something other than itself), and every builder of tests/gather_inputs.py shown to
make the case it is named for."""
import numpy as np

import gather_inputs as GI
import gather_restate as GR
from kspider_amd import engine

# (query, rank, source, overlap, unique, remaining), by hand
BY_HAND = {
    "tie_in_round_1": [(0, 1, 1, 3, 3, 4), (0, 2, 2, 3, 3, 1), (0, 3, 0, 1, 1, 0)],
    "tie_in_round_2": [(0, 1, 0, 5, 5, 6), (0, 2, 1, 4, 3, 3), (0, 3, 2, 3, 3, 0)],
    "subset_is_never_reported": [(0, 1, 1, 4, 4, 1), (0, 2, 2, 1, 1, 0)],
    "identical_sources": [(0, 1, 0, 3, 3, 1)],
    "falls_below_before_it_wins": [(0, 1, 0, 4, 4, 2)],
    "threshold_minus_1_and_exact": [(0, 1, 0, 5, 5, 5), (0, 2, 2, 4, 3, 2)],
    "empties_and_extreme_keys": [(1, 1, 1, 2, 2, 1), (3, 1, 1, 1, 1, 0)],
    "max_matches_1": [(0, 1, 0, 3, 3, 3)],
    "max_matches_2": [(0, 1, 0, 3, 3, 3), (0, 2, 1, 2, 2, 1)],
}


def _u(db, q_run, taken):
    """u(s) of every source for the query once the sources of `taken` were removed"""
    left = set(q_run) - set().union(*[set(db[s]) for s in taken]) if taken else set(q_run)
    return [len(set(s) & left) for s in db]


def test_hand_made_rows_are_what_the_restatement_gives():
    cases = GI.hand_made_cases()
    assert sorted(cases) == sorted(BY_HAND)
    for name, (db, q, m, k) in cases.items():
        assert GR.gather(db, q, m, k) == BY_HAND[name], name


def test_hand_made_cases_are_what_their_names_say():
    c = GI.hand_made_cases()
    db, q, _, _ = c["tie_in_round_1"]
    assert _u(db, q[0], [])[1] == _u(db, q[0], [])[2] == max(_u(db, q[0], []))                 # the tie is a tie, and it is the maximum
    db, q, _, _ = c["tie_in_round_2"]
    u1, u2 = _u(db, q[0], []), _u(db, q[0], [0])
    assert len(set(u1)) == 3 and u1[0] == max(u1) and u2[1] == u2[2] == 3                       # no tie in round 1, one in round 2
    db, q, _, _ = c["subset_is_never_reported"]
    assert set(db[0]) < set(db[1]) and all(r[2] != 0 for r in BY_HAND["subset_is_never_reported"])
    db, q, _, _ = c["identical_sources"]
    assert db[0] == db[1]
    db, q, m, _ = c["falls_below_before_it_wins"]
    counts = {}
    GR.gather(db, q, m, 0, counts)
    assert _u(db, q[0], [])[1] >= m > _u(db, q[0], [0])[1] and counts["fell_below"] == 1 and counts["candidates"] == 2
    db, q, m, _ = c["threshold_minus_1_and_exact"]
    assert _u(db, q[0], [0])[1] == m - 1 and _u(db, q[0], [0])[2] == m
    db, q, _, _ = c["empties_and_extreme_keys"]
    assert db[0] == [] and q[0] == [] and not (set(q[2]) & set().union(*map(set, db))) and 0 in db[1] and GI.TOP in db[1]


def test_generated_cases_are_what_their_names_say():
    db, q, m, _ = GI.shared_words_case()
    rows = GR.gather(db, q, m)
    assert len(q) == 40 and all(len(r) == 2 and 42 in r for r in q)
    assert rows == [(i, rank, rank - 1, 1, 1, 2 - rank) for i in range(40) for rank in (1, 2)]    # every query takes in both rounds
    db, q, m, _ = GI.chain_case()
    counts = {}
    rows = GR.gather(db, q, m, 0, counts)
    unique = [r[4] for r in rows]
    assert len(rows) == 70 and [r[2] for r in rows] == list(range(70)) and all(a > b for a, b in zip(unique, unique[1:])) and unique[-1] == 3 == m
    assert rows[1][3] == rows[1][4] + 5 and counts["iterations"] == [71] and rows[-1][5] == 0
    for cut in (15, 16, 17, 33):
        assert GR.gather(*GI.chain_case(max_matches=cut)) == rows[:cut]
    db, q, m, _ = GI.finish_case()
    assert [sum(r[0] == i for r in GR.gather(db, q, m)) for i in range(3)] == [0, 1, 40]
    db, q, m, _ = GI.segment_case()
    overlaps = [len(set(s) & set(q[0])) for s in db]
    rows = GR.gather(db, q, m)
    assert tuple(overlaps[:6]) == GI.SEGMENT_LENGTHS and overlaps[6] == 18 and sorted(r[2] for r in rows) == list(range(6)) and rows[-1][5] == 2
    for n_q in (3, 5):
        db, q, m, _ = GI.tiles_case(n_q)
        rows = GR.gather(db, q, m)
        assert len(q) == n_q and all(sum(r[0] == i for r in rows) >= 3 for i in range(n_q))
        assert any(r[3] != r[4] for r in rows)                                                     # matches hide each other
    db, q, m, _ = GI.sample_case()
    counts = {}
    rows = GR.gather(db, q, m, 0, counts)
    assert len(db) == 100 and len(q) == 1 and len(rows) >= 10 and counts["candidates"] > len(rows) and rows[-1][5] >= 1900   # the noise stays
    dk, do, qk, qo = GI.arrays(db, q)
    assert do.size == 101 and qo.size == 2 and int(qo[-1]) == qk.size and (np.diff(qk.astype(object)) > 0).all()


def test_python_mirror_of_the_row_and_stats_layout():
    assert engine.GATHER_ROW_DTYPE.itemsize == 24 and engine.GATHER_ROW_DTYPE.names == ("query", "rank", "source", "overlap", "unique", "remaining")
    import ctypes
    assert ctypes.sizeof(engine.GatherStats) == 176
    for name in ("ksp_gather_device", "ksp_gather_host", "kspider_gather"):
        assert name in engine.ABI_SYMBOLS and hasattr(engine.lib(), name)

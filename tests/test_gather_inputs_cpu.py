"""The gather tests' inputs and their restatement, checked without a GPU: the hand-made cases against rows written out by hand
(so that tests/gather_restate.py is pinned by something other than itself), and every builder of tests/gather_inputs.py shown to
make the case it is named for."""
import numpy as np

import gather_inputs as GI
import gather_restate as GR
import query_inputs
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


def _touched(db, q):
    """per database source: the queries it shares a key with"""
    return [sum(bool(set(int(k) for k in s) & set(int(k) for k in r)) for r in q) for s in db]


def test_wide_case_outgrows_the_list_the_first_buffer_and_the_tail_workgroup():
    db, q, m, k = GI.wide_case()
    counts = {}
    rows = GR.gather(db, q, m, k, counts)
    per_query = [sum(r[0] == j for r in rows) for j in range(len(q))]
    assert len(q) == 1100 and len(db) == 5 and (m, k) == (2, 0)
    assert len(rows) == 4051 and (per_query.count(3), per_query.count(4)) == (349, 751)
    assert (counts["candidates"], counts["dropped"], counts["fell_below"], max(counts["iterations"])) == (5311, 189, 1260, 5)
    assert sum(r[4] < r[3] for r in rows) == 1829                                               # matches hide each other
    assert GI.slots(db, q, m) == 19974 and sum(len(set(r)) for r in q) == 16216                 # (every key of a query is a holder)
    assert counts["candidates"] > max(engine.GATHER_FIRST_CANDS, 4 * len(db))                   # the candidate buffer regrows
    assert counts["candidates"] > engine.GATHER_TAIL_CANDS                                      # by default the batches do the rounds
    assert _touched(db, q) == [len(q)] * len(db) and len(q) > engine.QUERY_LIST_MAX             # every source overflows the list
    assert 1024 < len(q) <= engine.QUERY_TILE_MAX                                               # one tile, the tail's loops trip twice
    assert max(counts["iterations"]) <= engine.GATHER_BATCH                                     # one batch finishes it
    # tiles of QUERY_LIST_MAX: the list exactly full; one more: over by one in the first tile
    assert _touched(db, q[:engine.QUERY_LIST_MAX]) == [engine.QUERY_LIST_MAX] * len(db)
    for tile in (engine.QUERY_LIST_MAX, engine.QUERY_LIST_MAX + 1):
        tiled, total = GI.by_tile((db, q, m, k), tile, GR.gather)
        assert tiled == rows and total["passes"] == 3 and total["candidates"] == 5311 and total["slots"] == 19974


def test_list_edge_case_has_a_candidate_a_dropped_and_an_untouched_source():
    for n_share in (31, 32, 33, 200):
        db, q, m, k = GI.list_edge_case(n_share)
        counts = {}
        assert GR.gather(db, q, m, k, counts) == [(j, 1, 0, 2, 2, 1) for j in range(n_share)]
        assert counts["candidates"] == n_share and counts["dropped"] == n_share and counts["fell_below"] == 0
        assert _touched(db, q) == [n_share, n_share, 0]
        assert all(len(set(db[0]) & set(r)) == 2 >= m > len(set(db[1]) & set(r)) == 1 for r in q)
        sk = query_inputs.concat(db, q)
        want = query_inputs.expected(sk, len(db), query_inputs.CROSS)
        assert query_inputs.expected_overflows(want, len(db), engine.QUERY_TILE_MAX, 32) == (2 if n_share > 32 else 0)


def test_seam_case_has_a_skipped_a_rowless_and_a_full_tile():
    db, q, m, k = GI.seam_case()
    held = set().union(*[set(int(v) for v in s) for s in db])
    assert [len(r) for r in q[:2]] == [0, 0] and len(q[6]) == 0 and len(q) == 7
    assert all(len(r) and not (set(r) & held) for r in q[2:4])
    rows, total = GI.by_tile((db, q, m, k), 2, GR.gather)
    assert rows == GR.gather(db, q, m, k) and {r[0] for r in rows} == {4, 5} and all(sum(r[0] == j for r in rows) >= 3 for j in (4, 5))
    assert total["passes"] == 2 and total["rounds"] == max(sum(r[0] == j for r in rows) for j in (4, 5)) + 1
    # the capacities of the seam test on tiles_case(5): the first tile's rows end strictly inside the table
    case = GI.tiles_case(5)
    rows = GR.gather(*case)
    r1 = sum(r[0] < 2 for r in rows)
    assert 1 < r1 and r1 + 1 < len(rows) - 1 and GI.by_tile(case, 2, GR.gather)[1]["passes"] == 3


def test_chain_of_16_ends_a_batch_with_no_candidate_left():
    for n, rounds in ((15, 16), (16, 17)):
        counts = {}
        rows = GR.gather(*GI.chain_case(n), counts)
        assert len(rows) == n == counts["candidates"] and counts["iterations"] == [rounds] and counts["fell_below"] == 0
    # one batch takes exactly the 16 candidates; they start in batches only under a tail threshold below 16 (the default is above)
    assert engine.GATHER_BATCH == 16 <= engine.GATHER_TAIL_CANDS


def test_first_candidate_capacity_is_the_header_s():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "..", "include", "kspider_amd.h")).read()
    assert [int(v) for v in re.findall(r"#define KSP_GATHER_FIRST_CANDS (\d+)u", header)] == [engine.GATHER_FIRST_CANDS]


def test_block_case_run_lengths_and_candidates():
    db, q, m, k = GI.block_case()
    assert tuple(len(np.unique(r)) for r in db) == query_inputs.BLOCK_RUN_LENGTHS == (255, 256, 257, 1023, 1024, 1025, 3)
    assert len(q) == 6 and all(len(np.unique(r)) == query_inputs.BLOCK_QUERY_LENGTH == 600 for r in q)
    assert max(int(r.max()) for r in db + q) < 4000
    overlaps = [[len(set(s.tolist()) & set(r.tolist())) for r in q] for s in db]
    assert all(max(row) >= m for row in overlaps)                             # every source is a candidate of some query
    rows = GR.gather(db, q, m, k)
    assert any(r[4] < r[3] for r in rows) and {r[0] for r in rows} == set(range(6))


def test_switch_cases_cover_what_they_are_drawn_for():
    cases = GI.switch_cases()
    assert len(cases) == 48
    seen = {name: set() for name, _ in GI.SWITCH_CHOICES}
    with_rows = top_rank = fell = dropped = hidden = empty_q = empty_db = rowless = uneven = 0
    for case, env in cases:
        db, q, m, k = case
        assert 1 <= len(db) <= 12 and 1 <= len(q) <= 9 and m in (1, 2, 3, 5) and k in (0, 1, 2) and all(len(r) <= 30 for r in db + q)
        assert sorted(env) == sorted(seen)
        for name, value in env.items():
            assert value in dict(GI.SWITCH_CHOICES)[name]
            seen[name].add(value)
        tile = int(env["KSP_QUERY_TILE"] or engine.QUERY_TILE_MAX)
        counts = {}
        rows = GR.gather(db, q, m, k, counts)
        tiled, total = GI.by_tile(case, tile, GR.gather)
        assert tiled == rows and all(total[name] == counts[name] for name in ("candidates", "dropped", "fell_below"))
        assert total["slots"] == GI.slots(db, q, m)
        with_rows += bool(rows)
        top_rank = max([top_rank] + [r[1] for r in rows])
        fell += counts["fell_below"]
        dropped += counts["dropped"]
        hidden += sum(r[4] < r[3] for r in rows)
        empty_q += sum(len(r) == 0 for r in q)
        empty_db += sum(len(r) == 0 for r in db)
        rowless += len(q) - len({r[0] for r in rows})
        uneven += len(q) > tile and len(q) % tile != 0
    assert all(seen[name] == set(values) for name, values in GI.SWITCH_CHOICES)                 # every value of every switch is drawn
    assert with_rows >= 40 and top_rank >= 4 and fell > 0 and dropped > 0 and hidden > 0
    assert empty_q > 0 and empty_db > 0 and rowless > 0 and uneven > 0


def test_python_mirror_of_the_row_and_stats_layout():
    assert engine.GATHER_ROW_DTYPE.itemsize == 24 and engine.GATHER_ROW_DTYPE.names == ("query", "rank", "source", "overlap", "unique", "remaining")
    import ctypes
    assert ctypes.sizeof(engine.GatherStats) == 176
    for name in ("ksp_gather_device", "ksp_gather_host", "kspider_gather"):
        assert name in engine.ABI_SYMBOLS and hasattr(engine.lib(), name)

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


# ---- the inputs of tests/test_gather_abund_paths_gpu.py

def _one_take_rows(case, multisets):
    """the restatement's rows of a one_take_per_query case: one row per query, which takes its multiset whole"""
    rows = WR.gather(*case)
    assert [(r[0], r[1], r[2], r[3], r[4], r[5]) for r in rows] == [(i, 1, i, len(v), len(v), 0) for i, v in enumerate(multisets)]
    for r, v in zip(rows, multisets):
        s = sorted(v)
        assert (r[6], r[8], r[9]) == (sum(v), sum(x * x for x in v), s[(len(s) - 1) // 2] + s[len(s) // 2])
    return rows


def test_every_multiset_of_the_zoo_ends_the_select_in_the_state_it_is_named_for():
    named = I.ties_named()
    kinds = ("inside", "last_low_byte", "last_top_byte", "last_then_top32", "first_copy", "zeros_then_1", "zeros_then_top32", "low_byte_only", "top_byte_only",
             "corner_00000000", "corner_00ff00ff", "corner_ff00ff00", "corner_ffffffff", "lane_bin_0", "lane_bin_1", "lane_bin_2", "lane_bin_3")
    assert sorted(named) == sorted(f"{kind}_{n}" for kind in kinds for n in I.ZOO_SIZES)
    for name, (values, want) in named.items():
        assert len(values) == int(name.rsplit("_", 1)[1]) > 64 and I.select_state(values) == want, name
    for n in I.ZOO_SIZES:
        k1, even = (n - 1) // 2, n % 2 == 0
        state = lambda kind: named[f"{kind}_{n}"][1]                         # noqa: E731
        middle = lambda kind: sorted(named[f"{kind}_{n}"][0])[k1:k1 + 2]     # noqa: E731
        assert state("inside") == ("again" if even else "odd", 2, 6)         # 2 < eq < n, 0 < r, r + 1 < eq
        s = sorted(named[f"inside_{n}"][0])
        assert s[0] < s[k1] < s[-1]
        for kind, same in (("last_low_byte", 0xFFFFFF00), ("last_top_byte", 0x00FFFFFF), ("last_then_top32", None)):
            assert state(kind) == ("above" if even else "odd", 2, 3)         # the run ends at k1, r > 0
            v, nxt = middle(kind)
            assert nxt > v and (nxt == TOP32 if same is None else (v ^ nxt) & same == 0)
        assert state("first_copy") == ("above" if even else "odd", 0, 1)
        s = sorted(named[f"first_copy_{n}"][0])
        assert s.count(s[k1 + 1]) == 3 and s[k1 + 1] > s[k1]
        assert state("zeros_then_1") == state("zeros_then_top32") == ("above" if even else "odd", k1, k1 + 1)
        assert middle("zeros_then_1") == [0, 1] and middle("zeros_then_top32") == [0, TOP32]
        assert len({x >> 8 for x in named[f"low_byte_only_{n}"][0]}) == 1 and len({x & 0xFFFFFF for x in named[f"top_byte_only_{n}"][0]}) == 1
        for kind in ("low_byte_only", "top_byte_only"):
            assert 2 <= state(kind)[2] < n
        for v in (0, 0x00FF00FF, 0xFF00FF00, TOP32):
            values = named[f"corner_{v:08x}_{n}"][0]
            assert set(values) <= set(I.CORNERS) and sorted(values)[k1] == v and state(f"corner_{v:08x}")[1] > 0
        for b in range(4):
            v = sorted(named[f"lane_bin_{b}_{n}"][0])[k1]
            assert [(v >> s) & 3 for s in (24, 16, 8, 0)] == [b] * 4
            for s in (24, 16, 8, 0):   # the lane's three other bins hold 1, 2 and 3 values under the digits chosen before (and on the top passes what else fell there)
                same_lane = [(x >> s) & 3 for x in named[f"lane_bin_{b}_{n}"][0] if x >> (s + 8) == v >> (s + 8) and (x >> s) & 0xFC == (v >> s) & 0xFC]
                counts = [same_lane.count(d) for d in range(4) if d != b]
                assert all(c >= w for c, w in zip(counts, (1, 2, 3))) and (s or counts == [1, 2, 3])
    # the sizes' even members give every branch by name; r + 1 == eq and r + 1 < eq with eq on both sides of c[2] are in
    assert {named[f"lane_bin_{b}_66"][1] for b in range(4)} == {("again", 1, 3), ("above", 1, 2), ("above", 2, 3)}


def test_the_random_part_of_the_zoo_and_the_bins_of_a_lane():
    rnd = I.ties_random()
    assert 90 <= len(rnd) <= 110
    assert {combo for _, _, combo in rnd} == {(m, scale, where) for m in (2, 3, 5) for scale in (1, 1 << 8, 1 << 16, 1 << 24) for where in range(4)}
    for values, alphabet, (m, scale, where) in rnd:
        assert set(values) <= set(alphabet) and 64 < len(values) and len(alphabet) == m and max(alphabet) <= TOP32
        assert all((x - alphabet[0]) % scale == 0 for x in alphabet)
        assert alphabet[0] == (0, 255, 2**24 - 1)[where] if where < 3 else alphabet[-1] == TOP32
    states = [I.select_state(v) for v, _, _ in rnd]
    assert {branch for branch, r, _ in states if r > 0} == {"odd", "again", "above"}
    assert any(2 < eq < len(v) for (_, _, eq), (v, _, _) in zip(states, rnd))
    # every bin of a lane is the chosen one on every pass: the digits of the lower middle values of the whole zoo
    chosen = {p: set() for p in range(4)}
    for values in [v for v, _ in I.ties_named().values()] + [v for v, _, _ in rnd]:
        s = sorted(values)
        for p in range(4):
            chosen[p].add((s[(len(s) - 1) // 2] >> (24 - 8 * p)) & 3)
    assert all(chosen[p] == {0, 1, 2, 3} for p in range(4))
    names, case = I.zoo_case()
    multisets = case[2]
    assert len(names) == len(multisets) == len(set(names)) <= engine.QUERY_TILE_MAX                     # one tile
    _one_take_rows(case, multisets)


def test_carry_sets_wrap_a_lane_s_low_word():
    assert I.WRAP_MIN ** 2 >= 2**63 > (I.WRAP_MIN - 1) ** 2
    sets = I.carry_sets()
    assert sorted(sets) == sorted(f"{kind}_{n}" for kind in ("top32", "distinct", "mixed") for n in I.CARRY_SIZES)
    rows = _one_take_rows(I.carry_case(), list(sets.values()))
    for (name, values), row in zip(sets.items(), rows):
        n = len(values)
        assert n > 64 and row[8] >> 64 >= 1, name
        big = [v for v in values if v >= I.WRAP_MIN]
        if name.startswith("top32"):
            assert set(values) == {TOP32} and row[8] >> 64 == n - 1
        elif name.startswith("distinct"):
            assert len(set(values)) == n == len(big) and row[8] >> 64 >= n // 2      # every square is 2^63 or more
        else:
            assert len(big) == (n + 1) // 2 and all(v < 2**16 for v in values if v < I.WRAP_MIN) and row[8] >> 64 >= len(big) // 2
    # 1 025 values are 16 or 17 per lane: the upper word is near 1 024, many wraps in every lane
    by_name = dict(zip(sets, rows))
    assert by_name["top32_1025"][8] >> 64 == 1024 and by_name["distinct_1025"][8] >> 64 >= 512 and by_name["mixed_1025"][8] >> 64 >= 256


def test_dead_slots_across_trips():
    pairs = I.dead_pairs()
    assert len(pairs) == 52 and {L for L, _ in pairs} == set(I.DEAD_L) and all(n < L for L, n in pairs)
    for L in I.DEAD_L:
        assert {n for l, n in pairs if l == L} == {n for n in I.DEAD_N + (L - 1,) if n < L}
    case = I.dead_case()
    db, q, a, m, k = case
    assert sum(len(run) for run in q) == 58597 and (m, k) == (1, 0)
    rows = WR.gather(*case)
    assert len(rows) == 2 * len(pairs)
    for i, (L, n) in enumerate(pairs):
        killer, block = rows[2 * i], rows[2 * i + 1]
        assert killer[:6] == (i, 1, 2 * i, L + 1, L + 1, n) and block[:6] == (i, 2, 2 * i + 1, L, L, 0)[:4] + (n, 0)
        assert block[6] == 3 * n * (n + 1) // 2 and block[9] == 3 * ((n + 1) // 2 + n // 2 + 1)
        assert killer[6] >= (L - n) * 2**31 and len(set(db[2 * i]) & set(db[2 * i + 1])) == L - n
        dead = [v for v in a[i][:L] if v >= 2**31]
        assert len(dead) == L - n and sorted(v for v in a[i][:L] if v < 2**31) == [3 * j for j in range(1, n + 1)]
    # dead slots in every trip of 256 of a long segment, so that the stores fall trips behind the loads
    L, n = 2049, 1
    i = pairs.index((L, n))
    assert all(sum(v >= 2**31 for v in a[i][t:t + 256]) > 200 for t in range(0, 2048, 256))
    # the same with ties among the survivors
    case = I.dead_ties_case()
    rows = WR.gather(*case)
    assert len(rows) == 2 * len(I.DEAD_TIES_PAIRS)
    for i, (L, n) in enumerate(I.DEAD_TIES_PAIRS):
        block = rows[2 * i + 1]
        survivors = [v for v in case[2][i][:L] if not 2**31 <= v < 2**31 + 1000]
        assert block[:6] == (i, 2, 2 * i + 1, L, n, 0) and len(survivors) == n > 64 and set(survivors) == set(I.DEAD_TIES_ALPHABET)
        branch, r, eq = I.select_state(survivors)
        assert r > 0 and 2 < eq < n
        assert block[6] == sum(survivors) and block[9] == sorted(survivors)[(n - 1) // 2] + sorted(survivors)[n // 2]
    assert {I.select_state([v for v in case[2][i][:L] if not 2**31 <= v < 2**31 + 1000])[0] for i, (L, _) in enumerate(I.DEAD_TIES_PAIRS)} >= {"odd", "again"}


def test_abundances_attached_to_the_unweighted_cases():
    import gather_inputs as GI
    case = I.with_abunds(GI.wide_case())
    db, q, a, m, k = case
    assert (db, q, m, k) == GI.wide_case() and [len(run) for run in a] == [len(run) for run in q]
    flat = [v for run in a for v in run]
    assert 0 in flat and 1 in flat and any(1 < v < 2**20 for v in flat) and {TOP32 - i for i in range(4)} <= set(flat)
    assert all(v < 2**20 or v > TOP32 - 4 for v in flat)
    key = q[0][0]
    assert len({a[j][q[j].index(key)] for j in range(len(q)) if key in q[j]}) > 1            # one hash, other values in other queries
    assert [r[:6] for r in WR.gather(*case)] == gather_restate.gather(db, q, m, k)
    assert I.with_abunds(GI.seam_case())[2][:2] == [[], []]

"""Weighted gather on the GPU, the paths tests/test_gather_abund_gpu.py does not reach (kspider_amd/csrc/gather.hip: gather_take<true>,
gather_median2, k_gather_habund; kspider_amd/csrc/sketch_pack.cpp): every end state of the radix select's tie
bookkeeping, a lane's own carry in the sum of squares, a compaction whose stores fall trips behind its loads, the weighted row
type through the unweighted call's overflow, regrowth, seam and no-candidate cases, and a 128-bit numerator in the file layer.
Everything is compared with == against tests/gather_abund_restate.py; the inputs are tests/gather_abund_inputs.py's, shown on the
CPU to make these cases by tests/test_gather_abund_inputs_cpu.py."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import gather_abund_inputs as I
import gather_abund_restate as WR
import gather_inputs as GI
import gather_restate as GR
from kspider_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 8   # guard rows behind a row buffer
COUNTED = ("candidates", "dropped", "fell_below", "slots")
#: tests/test_gather_abund_gpu.py's
SWITCHES = [{"KSP_QUERY_TILE": "1"}, {"KSP_QUERY_TILE": "2", "KSP_GATHER_TAIL": "0"}, {"KSP_GATHER_TAIL": "0"}, {"KSP_GATHER_TAIL": "1", "KSP_GATHER_TAIL_CANDS": "1048576"},
            {"KSP_GATHER_MAX_WORKGROUPS": "1"}, {"KSP_GATHER_MAX_WORKGROUPS": "1", "KSP_GATHER_TAIL": "0", "KSP_GATHER_LONG_SEG": "4"},
            {"KSP_GATHER_TAIL_CANDS": "0"}, {"KSP_QUERY_TILE": "3", "KSP_QUERY_LIST": "1", "KSP_QUERY_LONG_RUN": "8"}]


def _tuples(rows):
    """the rows as the restatement writes them: the two words of the sum of squares joined"""
    return [tuple(int(r[n]) for n in ("query", "rank", "source", "overlap", "unique", "remaining", "w_unique", "w_found")) + ((int(r["sq_hi"]) << 64) | int(r["sq_lo"]), int(r["median2"]))
            for r in rows]


def _run(case):
    db, q, a, m, k = case
    dk, do, qk, qa, qo = I.arrays(db, q, a)
    got, st = engine.gather_abund_host(dk, do, qk, qa, qo, min_hashes=m, max_matches=k)
    plain, _ = engine.gather_host(dk, do, qk, qo, min_hashes=m, max_matches=k)
    assert [r[:6] for r in _tuples(got)] == [tuple(int(v) for v in r) for r in plain.tolist()]      # the first six fields are the unweighted call's
    return _tuples(got), st


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, the restatement's rows, a name per query), made once"""
    if name == "zoo":
        names, case = I.zoo_case()
    else:
        case = {"carries": I.carry_case, "dead": I.dead_case, "dead_ties": I.dead_ties_case}[name]()
        names = {"carries": list(I.carry_sets()), "dead": [f"L{L}_n{n}" for L, n in I.dead_pairs()], "dead_ties": [f"L{L}_n{n}" for L, n in I.DEAD_TIES_PAIRS]}[name]
    return case, WR.gather(*case), names


def _wrong(got, want, names):
    """the queries whose rows differ, by name"""
    rows = lambda table, q: [r for r in table if r[0] == q]   # noqa: E731
    return [(names[q], rows(got, q), rows(want, q)) for q in range(len(names)) if rows(got, q) != rows(want, q)][:4]


# ------------------------------------------------------------------------------------ A, B, C: the select, the carries, dead slots
def test_every_end_state_of_the_select():
    """232 queries of one tile, each one take of 65 .. 1 025 values: both middle ranks inside a run, a run that ends at the lower
    middle rank (the upper value one up in the lowest byte, in the top byte, 2^32 - 1), a run that starts at the upper one, zeros
    up to the lower one, values in one bin on three passes, bytes of 0x00 and 0xFF, each bin of a histogram lane chosen on every
    pass with the lane's other bins filled, and 96 seeded multisets over alphabets of 2, 3 and 5 values"""
    case, want, names = _case("zoo")
    got, st = _run(case)
    assert not _wrong(got, want, names)
    assert got == want and st["passes"] == 1 and st["rows"] == len(names)


def test_a_lane_adds_squares_that_wrap_its_low_word():
    """takes of 65, 128, 129 and 1 025 values of 3 037 000 500 or more: two squares of one lane pass 2^64"""
    case, want, names = _case("carries")
    got, _ = _run(case)
    assert not _wrong(got, want, names)
    assert got == want and all(r[8] >> 64 >= 1 for r in got)


@pytest.mark.parametrize("name", ["dead", "dead_ties"])
def test_dead_slots_across_the_trips_of_the_compaction(name):
    """segments of 257 .. 2 049 slots of which 1 .. L - 1 are alive when they are taken, the dead ones spread at random and heavy:
    the survivors are stored trips behind the loads, ranked in registers (up to 64) or selected by digits on the compacted front"""
    case, want, names = _case(name)
    got, st = _run(case)
    assert not _wrong(got, want, names)
    assert got == want and st["rows"] == 2 * len(names)


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "-".join(f"{k[4:]}={v}" for k, v in s.items()))
def test_the_same_rows_under_every_switch(monkeypatch, switches):
    """tiles of one, two and three queries, rounds in batches to the end and in the one-workgroup tail from the first round on, one
    workgroup for everything, segments of 4 slots or more counted by a workgroup"""
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    for name in ("zoo", "carries", "dead", "dead_ties"):
        case, want, names = _case(name)
        got, st = _run(case)
        assert not _wrong(got, want, names), name
        assert got == want, name
        if switches.get("KSP_GATHER_TAIL") == "0":
            assert st["tail_rounds"] == 0
        if "KSP_GATHER_TAIL_CANDS" in switches and switches["KSP_GATHER_TAIL_CANDS"] != "0":
            assert st["tail_rounds"] == st["rounds"] > 0
        if "KSP_GATHER_LONG_SEG" in switches:
            assert st["long_seg"] == 4


# ------------------------------------------------------------------------------------ D: the unweighted path cases, weighted
@pytest.fixture(scope="module")
def wide():
    case = I.with_abunds(GI.wide_case())
    _, total = GI.by_tile(GI.wide_case(), engine.QUERY_TILE_MAX, GR.gather)
    return case, WR.gather(*case), total


def _plain(case):
    return case[0], case[1], case[3], case[4]


@pytest.mark.parametrize("tail_cands", [None, "100000"])
@pytest.mark.parametrize("long_run", ["1", "100000"])
def test_wide_tile_overflows_the_list_and_outgrows_the_first_candidate_buffer(monkeypatch, wide, long_run, tail_cands):
    """1 100 queries in one tile that every source shares keys with: holder lists of 1 100 in k_gather_habund's search, the touched
    list replaced by the scan over all counters in both sweeps, the candidate buffer regrown, the tail wider than its threads"""
    case, want, total = wide
    assert total["candidates"] > max(engine.GATHER_FIRST_CANDS, 4 * len(case[0])) and len(case[1]) > engine.QUERY_LIST_MAX
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    if tail_cands:
        monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", tail_cands)
    got, st = _run(case)
    assert got == want
    assert {name: st[name] for name in COUNTED} == {name: total[name] for name in COUNTED}
    assert st["rounds"] == 5 == total["rounds"] and st["passes"] == 1 and st["rows"] == len(want)
    assert st["tail_rounds"] == (5 if tail_cands else 0) and st["batches"] == (0 if tail_cands else 1)
    assert st["live_at_tail"] == (total["candidates"] if tail_cands else 0)


@pytest.mark.parametrize("tile", [engine.QUERY_LIST_MAX, engine.QUERY_LIST_MAX + 1])
def test_wide_case_in_tiles_of_the_list_capacity_and_one_more(monkeypatch, wide, tile):
    """holder lists of 512 and 513 (and 75 in the last tile)"""
    case, want, _ = wide
    _, total = GI.by_tile(_plain(case), tile, GR.gather)
    monkeypatch.setenv("KSP_QUERY_TILE", str(tile))
    got, st = _run(case)
    assert got == want
    assert {name: st[name] for name in COUNTED + ("passes", "rounds")} == {name: total[name] for name in COUNTED + ("passes", "rounds")}
    assert st["passes"] == 3 and st["tile"] == tile


def test_wide_case_on_one_workgroup_per_grid(monkeypatch, wide):
    case, want, total = wide
    monkeypatch.setenv("KSP_GATHER_MAX_WORKGROUPS", "1")
    got, st = _run(case)
    assert got == want and st["rounds"] == 5 and st["candidates"] == total["candidates"] and st["slots"] == total["slots"]


@pytest.mark.parametrize("long_run", ["1", "100000"])
@pytest.mark.parametrize("n_share", [31, 32, 33, 200])
def test_touched_list_edge_in_both_sweeps(monkeypatch, n_share, long_run):
    case = I.with_abunds(GI.list_edge_case(n_share))
    monkeypatch.setenv("KSP_QUERY_LIST", "32")
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    got, st = _run(case)
    assert got == WR.gather(*case) and [r[:6] for r in got] == [(j, 1, 0, 2, 2, 1) for j in range(n_share)]
    assert st["candidates"] == n_share and st["dropped"] == n_share and st["fell_below"] == 0 and st["slots"] == 2 * n_share


def test_alive_bits_of_forty_queries_in_shared_words():
    case = I.with_abunds(GI.shared_words_case())
    got, _ = _run(case)
    assert got == WR.gather(*case) and len(got) == 80


def _device(case, capacity):
    """ksp_gather_abund_device with GUARD rows of a pattern behind the capacity: (rc, n, stats, the first `capacity` rows, guard intact)"""
    db, q, a, m, k = case
    dk, do, qk, qa, qo = I.arrays(db, q, a)
    bufs = [engine.DeviceBuffer.from_numpy(x) for x in (dk, qk, qa)]
    fill = np.full((capacity + GUARD) * 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_rows = engine.DeviceBuffer.from_numpy(fill)
    try:
        rc, n, st = engine.gather_abund_device(bufs[0].ptr, do, bufs[1].ptr, bufs[2].ptr, qo, d_rows.ptr, capacity, min_hashes=m, max_matches=k)
        back = d_rows.to_numpy(np.uint64, fill.size)
    finally:
        for b in bufs + [d_rows]:
            b.free()
    return rc, n, st, _tuples(back[:8 * capacity].view(engine.GATHER_WROW_DTYPE)), bool((back[8 * capacity:] == fill[8 * capacity:]).all())


def test_capacities_at_the_tile_seams_of_the_device_entry(monkeypatch):
    case = I.with_abunds(GI.tiles_case(5))
    want = WR.gather(*case)
    needed, r1 = len(want), sum(r[0] < 2 for r in want)
    monkeypatch.setenv("KSP_QUERY_TILE", "2")                                      # tiles of 2 + 2 + 1 queries
    for capacity in (0, r1 - 1, r1, r1 + 1, needed - 1, needed):
        rc, n, st, rows, guard = _device(case, capacity)
        assert n == needed and st["rows"] == needed and st["passes"] == 3, capacity
        assert rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW), capacity
        assert rows == want[:capacity], capacity                                   # the first rows, by (query, rank): w_found restarts per query
        assert guard, capacity                                                     # nothing behind the capacity, in rows of 64 bytes


def test_empty_and_rowless_tiles_before_a_tile_with_rows(monkeypatch):
    """qwfound is cleared where the segments are made, which a tile without an entry or without a candidate skips"""
    case = I.with_abunds(GI.seam_case())
    monkeypatch.setenv("KSP_QUERY_TILE", "2")
    want = WR.gather(*case)
    _, total = GI.by_tile(_plain(case), 2, GR.gather)
    assert {r[0] for r in want} == {4, 5}
    got, st = _run(case)
    assert got == want
    assert st["passes"] == 2 == total["passes"] and st["rounds"] == total["rounds"] and {name: st[name] for name in COUNTED} == {name: total[name] for name in COUNTED}
    rc, n, st, rows, guard = _device(case, len(want))
    assert (rc, n) == (engine.KSP_OK, len(want)) and rows == want and guard
    assert st["passes"] == 2 and st["rounds"] == total["rounds"]
    rc, n, _, rows, guard = _device(case, len(want) - 1)
    assert (rc, n) == (engine.KSP_E_OVERFLOW, len(want)) and rows == want[:-1] and guard


@pytest.mark.parametrize("tail", ["1", "0"])
def test_last_round_of_a_batch_takes_the_last_candidate(monkeypatch, tail):
    """chain_case(16): the weighted tail entered with no candidate left, or a second batch over two empty lists"""
    monkeypatch.setenv("KSP_GATHER_TAIL", tail)
    monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", "0")
    case = I.with_abunds(GI.chain_case(16))
    got, st = _run(case)
    assert got == WR.gather(*case) and len(got) == 16
    assert st["rounds"] == 17 and st["live_at_tail"] == 0 and st["candidates"] == 16
    assert (st["batches"], st["tail_rounds"]) == ((1, 1) if tail == "1" else (2, 0))


@pytest.mark.parametrize("long_run", ["1", "1000", "100000"])
def test_source_runs_at_the_probe_block(monkeypatch, long_run):
    case = I.with_abunds(GI.block_case())
    want = WR.gather(*case)
    _, total = GI.by_tile(_plain(case), engine.QUERY_TILE_MAX, GR.gather)
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    got, st = _run(case)
    assert got == want and len(got) >= 6
    assert {name: st[name] for name in COUNTED + ("rounds",)} == {name: total[name] for name in COUNTED + ("rounds",)}


def test_random_switches_on_random_small_cases(monkeypatch):
    names = [name for name, _ in GI.SWITCH_CHOICES]
    for number, (plain, env) in enumerate(GI.switch_cases()):
        for name in names:
            if env[name] is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, env[name])
        case = I.with_abunds(plain, seed=100 + number)
        tile = int(env["KSP_QUERY_TILE"] or engine.QUERY_TILE_MAX)
        _, total = GI.by_tile(plain, tile, GR.gather)
        what = f"case {number}: n_db {len(plain[0])}, n_q {len(plain[1])}, min_hashes {plain[2]}, max_matches {plain[3]}, {env}"
        want = WR.gather(*case)
        got, st = _run(case)
        assert got == want, what
        for name in COUNTED + ("passes", "rounds"):
            assert st[name] == total[name], f"{what}: {name} {st[name]}, expected {total[name]}"
        assert st["rows"] == len(want), what


# ------------------------------------------------------------------------------------ E: the file layer's 128-bit numerator
K, TOP32 = 21, I.TOP32
HEADER = ("query\trank\tmatch\toverlap\tunique\tf_orig_query\tf_unique_to_query\tf_match\tremaining\tf_unique_weighted\taverage_abund\tmedian_abund\tstd_abund\t"
          "n_unique_weighted_found\tsum_weighted_found\ttotal_weighted_hashes\n")


def _sig(path, mins, abunds=None):
    sig = {"ksize": K, "mins": [int(m) for m in mins]}
    if abunds is not None:
        sig["abundances"] = [int(a) for a in abunds]
    path.write_text(json.dumps([{"class": "sourmash_signature", "signatures": [sig]}]))


def test_signatures_with_abundances_up_to_the_clamp(tmp_path):
    """Signatures written here as JSON.  Query q0 takes 140 000 hashes whose abundances are 0 .. 3 and 2^32 - 4 .. 2^32 - 1 (n Σa² -
    (Σa)² above 2^96), then five of 2^32 - 1 (exactly 0; the sum of squares in two words), then (0, 0, 2^32 - 1): above 2^64.  q1
    lists a hash twice, 2^32 - 2 and 3: the sum clamps.  q2's abundances are all 0: W = 0."""
    rng = np.random.default_rng(17)
    big = [int(h) for h in np.unique(rng.integers(0, 2**64, size=140000, dtype=np.uint64))]
    five, three, dup = [2**64 - 1 - i for i in range(5)], [7, 8, 9], [100, 101, 102]
    db = {"d0": big, "d1": five, "d2": three, "d3": dup + [5000], "d4": [1, 2]}
    big_abunds = [int(v) if v < 4 else TOP32 - int(v - 4) for v in rng.integers(0, 8, size=len(big))]
    queries = {"q0": (big + five + three, big_abunds + [TOP32] * 5 + [0, 0, TOP32]), "q1": ([100, 101, 100, 102], [TOP32 - 1, 7, 3, 9]),
               "q2": (three + [77], [0, 0, 0, 0])}
    merged = {"q0": queries["q0"], "q1": ([100, 101, 102], [TOP32, 7, 9]), "q2": queries["q2"]}          # as the reader hands them on
    (tmp_path / "db").mkdir()
    (tmp_path / "q").mkdir()
    for name, mins in db.items():
        _sig(tmp_path / "db" / (name + ".sig"), mins)
    for name, (mins, abunds) in queries.items():
        _sig(tmp_path / "q" / (name + ".sig"), mins, abunds)
    mins, abunds = engine.sig_read(str(tmp_path / "q" / "q1.sig"), K)
    assert (mins.tolist(), abunds.tolist()) == merged["q1"]
    db_names, q_names = sorted(db), sorted(queries)
    q, a = [merged[n][0] for n in q_names], [merged[n][1] for n in q_names]
    rows = WR.gather([db[n] for n in db_names], q, a, 1, 0)
    spread = {(q_names[r[0]], db_names[r[2]]): r[4] * r[8] - r[6] * r[6] for r in rows}
    assert spread["q0", "d0"] > 2**96 and spread["q0", "d2"] > 2**64 and spread["q0", "d1"] == 0 and spread["q2", "d2"] == 0
    assert [(q_names[r[0]], db_names[r[2]]) for r in rows] == [("q0", "d0"), ("q0", "d1"), ("q0", "d2"), ("q1", "d3"), ("q2", "d2")]
    text = HEADER
    for row in rows:
        query, rank, source, overlap, unique, remaining, w_unique, w_found = row[:8]
        W = sum(a[query])
        floats = [np.float32(overlap) / np.float32(len(q[query])), np.float32(unique) / np.float32(len(q[query])), np.float32(overlap) / np.float32(len(db[db_names[source]]))]
        weighted = [np.float32(v) for v in WR.columns(row, W)]
        text += "\t".join([q_names[query], str(rank), db_names[source], str(overlap), str(unique)] + [engine.format_float(float(v)) for v in floats] + [str(remaining)]
                          + [engine.format_float(float(v)) for v in weighted] + [str(w_unique), str(w_found), str(W)]) + "\n"
    out = str(tmp_path / "OUT")
    engine.gather_abund(str(tmp_path / "db"), str(tmp_path / "q"), K, out, 2)
    got = open(out + "_kSpider_gather.tsv", "rb").read()
    assert got.decode().splitlines() == text.splitlines()
    assert got == text.encode()
    done = subprocess.run([os.path.join(os.path.dirname(engine.LIB_PATH), "gather"), str(tmp_path / "db"), str(tmp_path / "q"), str(K), out + "_tool", "2", "1", "--abund"],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert open(out + "_tool_kSpider_gather.tsv", "rb").read() == text.encode()

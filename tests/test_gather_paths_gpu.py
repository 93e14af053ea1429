"""Gather on the GPU, the paths tests/test_gather_gpu.py does not reach (kspider_amd/csrc/gather.hip, csrc/query_table.hip.h;
DESIGN.md 7o): the touched list overflowing in the counting and in the filling sweep, the candidate buffer outgrown and the
counting sweep run twice, a tile wider than the tail's 1 024 threads, tile seams on the device entry, the tail and a batch with no
candidate left, source runs at the probe block, and the switches in random combination.  Everything is compared with == against
tests/gather_restate.py; the inputs are tests/gather_inputs.py's, shown on the CPU to make these cases by
tests/test_gather_inputs_cpu.py."""
import numpy as np
import pytest

import gather_inputs as GI
import gather_restate as GR
from kspider_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 16   # guard rows behind a row buffer
SWITCHES = [name for name, _ in GI.SWITCH_CHOICES]
COUNTED = ("candidates", "dropped", "fell_below", "slots")


def _tuples(rows):
    return [tuple(int(v) for v in r) for r in rows.tolist()]


def _host(case):
    db, q, m, k = case
    got, st = engine.gather_host(*GI.arrays(db, q), min_hashes=m, max_matches=k)
    return _tuples(got), st


def _device(case, capacity, with_buffer=True):
    """ksp_gather_device with GUARD rows of a pattern behind the capacity: (rc, n, stats, the first `capacity` rows, guard intact)"""
    db, q, m, k = case
    dbk, dbo, qk, qo = GI.arrays(db, q)
    d_db, d_q = engine.DeviceBuffer.from_numpy(dbk), engine.DeviceBuffer.from_numpy(qk)
    fill = np.full((capacity + GUARD) * 6, 0xA5A5A5A5, dtype=np.uint32)
    d_rows = engine.DeviceBuffer.from_numpy(fill) if with_buffer else None
    try:
        rc, n, st = engine.gather_device(d_db.ptr, dbo, d_q.ptr, qo, d_rows.ptr if d_rows else None, capacity, min_hashes=m, max_matches=k)
        back = d_rows.to_numpy(np.uint32, fill.size) if d_rows else fill
    finally:
        for b in (d_db, d_q, d_rows):
            if b:
                b.free()
    return rc, n, st, _tuples(back[:6 * capacity].view(engine.GATHER_ROW_DTYPE)), bool((back[6 * capacity:] == fill[6 * capacity:]).all())


@pytest.fixture(scope="module")
def wide():
    case = GI.wide_case()
    rows, total = GI.by_tile(case, engine.QUERY_TILE_MAX, GR.gather)
    return case, rows, total


# ------------------------------------------------------------------------------------ 1. overflow, regrowth and a wide tile
@pytest.mark.parametrize("tail_cands", [None, "100000"])
@pytest.mark.parametrize("long_run", ["1", "100000"])
def test_wide_tile_overflows_the_list_and_outgrows_the_first_candidate_buffer(monkeypatch, wide, long_run, tail_cands):
    """1 100 queries in one tile, every source shares keys with all of them: both sweeps replace the touched list by the scan over
    all counters (512 < 1 100), the 5 311 candidates do not fit the first buffer (the counting sweep runs twice), and the tail's
    hand-over count and take loop trip twice.  Workgroup sweeps (long_run 1) and wave sweeps; rounds in a batch, or all in the tail."""
    case, want, total = wide
    assert total["candidates"] > max(engine.GATHER_FIRST_CANDS, 4 * len(case[0])) and len(case[1]) > engine.QUERY_LIST_MAX
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    if tail_cands:
        monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", tail_cands)
    got, st = _host(case)
    assert got == want
    assert {name: st[name] for name in COUNTED} == {name: total[name] for name in COUNTED}
    assert st["rounds"] == 5 == total["rounds"] and st["passes"] == 1 and st["rows"] == len(want)
    assert st["tail_rounds"] == (5 if tail_cands else 0) and st["batches"] == (0 if tail_cands else 1)
    assert st["live_at_tail"] == (total["candidates"] if tail_cands else 0)


@pytest.mark.parametrize("tile", [engine.QUERY_LIST_MAX, engine.QUERY_LIST_MAX + 1])
def test_wide_case_in_tiles_of_the_list_capacity_and_one_more(monkeypatch, wide, tile):
    """a tile of 512: every source's list is exactly full; 513: over by one in the first tile (and in the second)"""
    case, want, _ = wide
    _, total = GI.by_tile(case, tile, GR.gather)
    monkeypatch.setenv("KSP_QUERY_TILE", str(tile))
    got, st = _host(case)
    assert got == want
    assert {name: st[name] for name in COUNTED + ("passes", "rounds")} == {name: total[name] for name in COUNTED + ("passes", "rounds")}
    assert st["passes"] == 3 and st["tile"] == tile


def test_wide_case_on_one_workgroup_per_grid(monkeypatch, wide):
    case, want, total = wide
    monkeypatch.setenv("KSP_GATHER_MAX_WORKGROUPS", "1")
    got, st = _host(case)
    assert got == want and st["rounds"] == 5 and st["candidates"] == total["candidates"] and st["slots"] == total["slots"]


def test_wide_case_overflows_query_mode_s_list_too(wide):
    """independent of gather: the same arrays under the same environment overflow the list of query mode's sweep, once per source"""
    case, _, _ = wide
    _, st = engine.query_host(*GI.arrays(case[0], case[1]))
    assert st["list_overflows"] == len(case[0]) == 5 and st["list_capacity"] == engine.QUERY_LIST_MAX


# ------------------------------------------------------------------------------------ 2. the list's capacity edge
@pytest.mark.parametrize("long_run", ["1", "100000"])
@pytest.mark.parametrize("n_share", [31, 32, 33, 200])
def test_touched_list_edge_in_both_sweeps(monkeypatch, n_share, long_run):
    case = GI.list_edge_case(n_share)
    monkeypatch.setenv("KSP_QUERY_LIST", "32")
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    got, st = _host(case)
    assert got == [(j, 1, 0, 2, 2, 1) for j in range(n_share)] == GR.gather(*case)
    assert st["candidates"] == n_share and st["dropped"] == n_share and st["fell_below"] == 0 and st["slots"] == 2 * n_share
    _, qst = engine.query_host(*GI.arrays(case[0], case[1]))
    assert qst["list_capacity"] == 32 and qst["list_overflows"] == (2 if n_share > 32 else 0)


# ------------------------------------------------------------------------------------ 3. tile seams
def test_capacities_at_the_tile_seams_of_the_device_entry(monkeypatch):
    case = GI.tiles_case(5)
    want = GR.gather(*case)
    needed, r1 = len(want), sum(r[0] < 2 for r in want)
    monkeypatch.setenv("KSP_QUERY_TILE", "2")                                      # tiles of 2 + 2 + 1 queries
    rc, n, st, _, _ = _device(case, 0, with_buffer=False)                          # the size query
    assert (rc, n, st["passes"]) == (engine.KSP_E_OVERFLOW, needed, 3)
    for capacity in (0, r1 - 1, r1, r1 + 1, needed - 1, needed):
        rc, n, st, rows, guard = _device(case, capacity)
        assert n == needed and st["rows"] == needed and st["passes"] == 3, capacity
        assert rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW), capacity
        assert rows == want[:capacity], capacity                                   # the first rows, by (query, rank)
        assert guard, capacity                                                     # nothing behind the capacity


def test_empty_and_rowless_tiles_before_a_tile_with_rows(monkeypatch):
    case = GI.seam_case()
    monkeypatch.setenv("KSP_QUERY_TILE", "2")
    want, total = GI.by_tile(case, 2, GR.gather)
    assert want == GR.gather(*case) and {r[0] for r in want} == {4, 5}             # the global query indices
    got, st = _host(case)
    assert got == want
    assert st["passes"] == 2 == total["passes"] and st["rounds"] == total["rounds"] and {name: st[name] for name in COUNTED} == {name: total[name] for name in COUNTED}
    rc, n, st, rows, guard = _device(case, len(want))
    assert (rc, n) == (engine.KSP_OK, len(want)) and rows == want and guard
    assert st["passes"] == 2 and st["rounds"] == total["rounds"]
    rc, n, _, rows, guard = _device(case, len(want) - 1)
    assert (rc, n) == (engine.KSP_E_OVERFLOW, len(want)) and rows == want[:-1] and guard


# ------------------------------------------------------------------------------------ 4. no candidate left
@pytest.mark.parametrize("tail", ["1", "0"])
def test_last_round_of_a_batch_takes_the_last_candidate(monkeypatch, tail):
    """chain_case(16): the first batch's 16 rounds take the 16 candidates, the query still counts once.  With the tail (its
    threshold under the 16 candidates, so that the batch runs first) it is entered with no candidate and a bound of one round;
    without it a second batch is launched over two empty lists.  chain_case(15) ends inside the batch either way."""
    monkeypatch.setenv("KSP_GATHER_TAIL", tail)
    monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", "0")
    case = GI.chain_case(16)
    got, st = _host(case)
    assert got == GR.gather(*case) and len(got) == 16
    assert st["rounds"] == 17 and st["live_at_tail"] == 0 and st["candidates"] == 16
    assert (st["batches"], st["tail_rounds"]) == ((1, 1) if tail == "1" else (2, 0))
    case = GI.chain_case(15)
    got, st = _host(case)
    assert got == GR.gather(*case) and len(got) == 15
    assert (st["rounds"], st["batches"], st["tail_rounds"], st["live_at_tail"]) == (16, 1, 0, 0)


# ------------------------------------------------------------------------------------ 5. run lengths at the probe block
@pytest.mark.parametrize("long_run", ["1", "1000", "100000"])
def test_source_runs_at_the_probe_block(monkeypatch, long_run):
    """runs of 255 / 256 / 257 and 1 023 / 1 024 / 1 025 entries through the counting walk and the filling walk: all by
    workgroups, the three longest by workgroups, all by waves"""
    case = GI.block_case()
    want, total = GI.by_tile(case, engine.QUERY_TILE_MAX, GR.gather)
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)
    got, st = _host(case)
    assert got == want and len(got) >= 6
    assert {name: st[name] for name in COUNTED + ("rounds",)} == {name: total[name] for name in COUNTED + ("rounds",)}


# ------------------------------------------------------------------------------------ 6. the switches in combination
def test_random_switches_on_random_small_cases(monkeypatch):
    for number, (case, env) in enumerate(GI.switch_cases()):
        for name in SWITCHES:
            if env[name] is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, env[name])
        tile = int(env["KSP_QUERY_TILE"] or engine.QUERY_TILE_MAX)
        want, total = GI.by_tile(case, tile, GR.gather)
        what = f"case {number}: n_db {len(case[0])}, n_q {len(case[1])}, min_hashes {case[2]}, max_matches {case[3]}, {env}"
        got, st = _host(case)
        assert got == want, what
        for name in COUNTED + ("passes", "rounds"):
            assert st[name] == total[name], f"{what}: {name} {st[name]}, expected {total[name]}"
        assert st["rows"] == len(want), what

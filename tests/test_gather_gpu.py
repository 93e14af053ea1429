"""Gather on the GPU (kspider_amd/csrc/gather.hip): ksp_gather_host and ksp_gather_device against the restatement in
Python sets (tests/gather_restate.py) — exact, compared with ==.  The inputs and what each is for: tests/gather_inputs.py (checked
on the CPU, against rows written out by hand, by tests/test_gather_inputs_cpu.py)."""
import numpy as np
import pytest

import gather_inputs as GI
import gather_restate as GR
from kspider_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 16   # guard rows behind a row buffer


def _tuples(rows):
    return [tuple(int(v) for v in r) for r in rows.tolist()]


def _run(case, counts=None):
    """(rows of ksp_gather_host as tuples, the restatement's rows, stats)"""
    db, q, m, k = case
    got, st = engine.gather_host(*GI.arrays(db, q), min_hashes=m, max_matches=k)
    return _tuples(got), GR.gather(db, q, m, k, counts), st


@pytest.fixture(scope="module")
def chain():
    case = GI.chain_case()
    return case, GR.gather(*case)


@pytest.fixture(scope="module")
def random_cases():
    out = {}
    for name, case in (("random", GI.random_case()), ("sample", GI.sample_case())):
        counts = {}
        out[name] = (case, GR.gather(*case, counts), counts)
    return out


@pytest.mark.parametrize("name", sorted(GI.hand_made_cases()))
def test_hand_made(name):
    counts = {}
    got, want, st = _run(GI.hand_made_cases()[name], counts)
    assert got == want
    assert st["rows"] == len(want) and st["candidates"] == counts["candidates"] and st["dropped"] == counts["dropped"] and st["fell_below"] == counts["fell_below"]
    if name == "falls_below_before_it_wins":
        assert st["fell_below"] == 1 and st["candidates"] == 2                     # dropped in a round, and counted
    if name == "empties_and_extreme_keys":
        assert st["passes"] == 1 and st["n_q"] == 4 and st["n_db"] == 4


def test_queries_that_share_alive_words():
    got, want, st = _run(GI.shared_words_case())
    assert got == want and len(got) == 80 and st["rounds"] == 3 and st["slots"] == 80 and st["table_holders"] == 80


def test_queries_that_finish_in_different_rounds():
    got, want, st = _run(GI.finish_case())
    assert got == want and st["rounds"] == 41 and [sum(r[0] == i for r in got) for i in range(3)] == [0, 1, 40]


@pytest.mark.parametrize("cut", [15, 16, 17, 33, 0])
def test_chain_cut_around_a_batch(monkeypatch, chain, cut):
    case, full = chain
    monkeypatch.setenv("KSP_GATHER_TAIL", "0")
    got, st = engine.gather_host(*GI.arrays(case[0], case[1]), min_hashes=case[2], max_matches=cut)
    want = full[:cut] if cut else full
    rounds = cut if cut else 71                                                    # a query stopped by max_matches is not counted again
    assert _tuples(got) == want
    assert st["rounds"] == rounds and st["tail_rounds"] == 0 and st["live_at_tail"] == 0 and st["batches"] == (rounds + engine.GATHER_BATCH - 1) // engine.GATHER_BATCH


@pytest.mark.parametrize("tail_cands, batches", [("1000", 0), ("40", 2), ("0", 5)])
def test_chain_enters_the_tail(monkeypatch, chain, tail_cands, batches):
    """70 candidates, 16 taken per batch: the tail is entered at once (1 000), after two batches (70 - 32 = 38 <= 40), or only once
    no candidate is live (after 5 batches = 80 rounds every query is finished: it never runs)."""
    case, full = chain
    monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", tail_cands)
    got, st = engine.gather_host(*GI.arrays(case[0], case[1]), min_hashes=case[2], max_matches=0)
    assert _tuples(got) == full
    assert st["rounds"] == 71 and st["batches"] == batches and st["tail_rounds"] == 71 - min(71, 16 * batches)
    assert st["live_at_tail"] == (70 - 16 * batches if batches < 5 else 0) and st["tail_cands"] == int(tail_cands)


@pytest.mark.parametrize("long_seg, n_long", [("256", 2), ("1", 7), ("100000", 0)])
@pytest.mark.parametrize("tail", ["0", "1"])
def test_segment_lengths(monkeypatch, long_seg, n_long, tail):
    monkeypatch.setenv("KSP_GATHER_LONG_SEG", long_seg)
    monkeypatch.setenv("KSP_GATHER_TAIL", tail)
    got, want, st = _run(GI.segment_case())
    assert got == want and st["long_seg"] == int(long_seg) and st["slots"] == sum(GI.SEGMENT_LENGTHS) + 18
    assert sum(n >= int(long_seg) for n in GI.SEGMENT_LENGTHS + (18,)) == n_long


@pytest.mark.parametrize("cap", [None, "1", "2"])
@pytest.mark.parametrize("n_q", [3, 5])
def test_tiles_and_grids(monkeypatch, n_q, cap):
    case = GI.tiles_case(n_q)
    whole, want, st_whole = _run(case)
    monkeypatch.setenv("KSP_QUERY_TILE", "2")
    monkeypatch.setenv("KSP_GATHER_TAIL", "0")
    monkeypatch.setenv("KSP_GATHER_LONG_SEG", "20")                                # both kinds of candidate
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", "40")                                 # every source long in the sweeps
    if cap:
        monkeypatch.setenv("KSP_GATHER_MAX_WORKGROUPS", cap)
    tiled, _, st = _run(case)
    assert whole == want and tiled == want
    assert st_whole["passes"] == 1 and st["passes"] == (n_q + 1) // 2 and st["tile"] == 2 and st["candidates"] == st_whole["candidates"] and st["slots"] == st_whole["slots"]


@pytest.mark.parametrize("cap", ["1", "2"])
def test_grids_on_the_random_case(monkeypatch, random_cases, cap):
    case, want, _ = random_cases["random"]
    monkeypatch.setenv("KSP_GATHER_MAX_WORKGROUPS", cap)
    monkeypatch.setenv("KSP_GATHER_LONG_SEG", "60")
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", "400")
    monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", "50")
    got, st = engine.gather_host(*GI.arrays(case[0], case[1]), min_hashes=case[2])
    assert _tuples(got) == want and st["batches"] >= 1


@pytest.mark.parametrize("name", ["random", "sample"])
@pytest.mark.parametrize("tail", ["0", "1"])
def test_random_cases_and_their_invariants(monkeypatch, random_cases, name, tail):
    case, want, counts = random_cases[name]
    db, q, m, _ = case
    monkeypatch.setenv("KSP_GATHER_TAIL", tail)
    monkeypatch.setenv("KSP_GATHER_TAIL_CANDS", "100000")                          # (when there is a tail, it is entered at once)
    arrays = GI.arrays(db, q)
    got, st = engine.gather_host(*arrays, min_hashes=m)
    assert _tuples(got) == want and len(got) >= 10
    assert st["candidates"] == counts["candidates"] and st["dropped"] == counts["dropped"] and st["fell_below"] == counts["fell_below"]
    assert st["rounds"] == max(counts["iterations"]) and st["tail_rounds"] == (0 if tail == "0" else st["rounds"])
    # independent of the restatement: rank 1 is the arg-max of query mode's shared counts, unique never rises, the sums close
    edges, _ = engine.query_host(*arrays)
    sizes = np.diff(arrays[3].astype(np.int64))
    for j in range(len(q)):
        mine = got[got["query"] == j]
        pairs = edges[edges["source_2"] == len(db) + j]
        if len(mine) == 0:
            assert len(pairs) == 0 or int(pairs["shared"].max()) < m
            continue
        top = int(pairs["shared"].max())
        first = int(pairs["source_1"][pairs["shared"] == top].min())
        assert (int(mine["rank"][0]), int(mine["source"][0]), int(mine["overlap"][0]), int(mine["unique"][0])) == (1, first, top, top)
        assert (np.diff(mine["unique"].astype(np.int64)) <= 0).all() and (mine["rank"] == np.arange(1, len(mine) + 1)).all()
        assert int(sizes[j]) - int(mine["unique"].sum()) == int(mine["remaining"][-1])


def test_device_entry_size_query_capacity_and_a_resident_database(random_cases):
    case, want, _ = random_cases["random"]
    dbk, dbo, qk, qo = GI.arrays(case[0], case[1])
    d_db, d_q = engine.DeviceBuffer.from_numpy(dbk), engine.DeviceBuffer.from_numpy(qk)
    needed = len(want)
    rc, n, _ = engine.gather_device(d_db.ptr, dbo, d_q.ptr, qo, None, 0, min_hashes=case[2])         # the size query
    assert (rc, n) == (engine.KSP_E_OVERFLOW, needed)
    fill = np.full((needed + GUARD) * 6, 0xA5A5A5A5, dtype=np.uint32)
    for capacity in (needed - 1, needed, needed):                                                    # the last: the same resident database again
        d_rows = engine.DeviceBuffer.from_numpy(fill)
        rc, n, st = engine.gather_device(d_db.ptr, dbo, d_q.ptr, qo, d_rows.ptr, capacity, min_hashes=case[2])
        assert n == needed and st["rows"] == needed
        assert rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW)
        back = d_rows.to_numpy(np.uint32, fill.size)
        assert (back[6 * capacity:] == fill[6 * capacity:]).all()                                    # nothing behind the capacity
        assert _tuples(back[:6 * capacity].view(engine.GATHER_ROW_DTYPE)) == want[:capacity]         # the first rows, in order
        d_rows.free()
    d_db.free()
    d_q.free()


def test_refusals_and_a_valid_call_after_them(monkeypatch):
    case = GI.hand_made_cases()["tie_in_round_2"]
    dbk, dbo, qk, qo = GI.arrays(case[0], case[1])
    d_db, d_q, d_rows = engine.DeviceBuffer.from_numpy(dbk), engine.DeviceBuffer.from_numpy(qk), engine.DeviceBuffer(24 * 64)
    z = np.zeros(1, np.uint64)
    ok = dict(d_db_keys_ptr=d_db.ptr, db_offsets=dbo, d_q_keys_ptr=d_q.ptr, q_offsets=qo, d_rows_ptr=d_rows.ptr, capacity=64, min_hashes=1)
    arg_cases = [("NULL argument", dict(d_db_keys_ptr=None)), ("NULL argument", dict(db_offsets=None)), ("NULL argument", dict(d_q_keys_ptr=None)),
                 ("NULL argument", dict(q_offsets=None)), ("d_rows is NULL but capacity is not 0", dict(d_rows_ptr=None)),
                 ("no database source or no query", dict(db_offsets=z)), ("no database source or no query", dict(q_offsets=z)),
                 ("min_hashes is 1 or more", dict(min_hashes=0)),
                 ("the database offsets do not start at 0", dict(db_offsets=dbo + 1)), ("the query offsets do not start at 0", dict(q_offsets=qo[::-1].copy())),
                 ("the database offsets decrease at source 1", dict(db_offsets=np.array([0, 5, 4, 9], dtype=np.uint64)))]
    for text, change in arg_cases:
        for device in (0, 99):                                                     # refused before a device is touched
            with pytest.raises(engine.KspError) as ei:
                engine.gather_device(**{**ok, **change}, device=device)
            assert ei.value.code == engine.KSP_E_ARG and f"ksp_gather_device: {text}" in str(ei.value), (text, device)
    with pytest.raises(engine.KspError) as ei:                                     # n_rows itself NULL
        engine._check(engine.lib().ksp_gather_device(99, d_db.ptr, dbo.ctypes.data, 3, d_q.ptr, qo.ctypes.data, 1, 1, 0, d_rows.ptr, 64, None, None))
    assert ei.value.code == engine.KSP_E_ARG and "NULL argument" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:                                     # ksp_gather_host: the rows pointer NULL
        engine._check(engine.lib().ksp_gather_host(dbk.ctypes.data, dbo.ctypes.data, 3, qk.ctypes.data, qo.ctypes.data, 1, 1, 0, 99, None, z.ctypes.data, None))
    assert ei.value.code == engine.KSP_E_ARG and "ksp_gather_host: NULL argument" in str(ei.value)
    for name, value in [("KSP_QUERY_TILE", "0"), ("KSP_QUERY_TILE", str(engine.QUERY_TILE_MAX + 1)), ("KSP_QUERY_LIST", "0"), ("KSP_QUERY_LONG_RUN", "many"),
                        ("KSP_GATHER_LONG_SEG", "0"), ("KSP_GATHER_LONG_SEG", str(2**32)), ("KSP_GATHER_TAIL", "2"), ("KSP_GATHER_TAIL", "yes"),
                        ("KSP_GATHER_TAIL_CANDS", str(engine.GATHER_TAIL_CANDS_MAX + 1)), ("KSP_GATHER_TAIL_CANDS", "-1")]:
        monkeypatch.setenv(name, value)
        with pytest.raises(engine.KspError) as ei:
            engine.gather_host(dbk, dbo, qk, qo, device=99)
        assert ei.value.code == engine.KSP_E_ARG and f"ksp_gather_host: {name} is a number from" in str(ei.value)
        monkeypatch.delenv(name)
    # KSP_E_LIMIT under query mode's limits: a tile of 2^31 entries, memory that cannot fit, 2^32 - 1 sources (from the counts alone)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_device(**{**ok, "q_offsets": np.array([0, 2**31], dtype=np.uint64)})
    assert ei.value.code == engine.KSP_E_LIMIT and "2^31" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_host(dbk, np.array([0, 2**40], dtype=np.uint64), qk, qo)
    assert ei.value.code == engine.KSP_E_LIMIT and "bytes of device memory" in str(ei.value) and "are free" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine._check(engine.lib().ksp_gather_device(99, d_db.ptr, dbo.ctypes.data, 2**32 - 2, d_q.ptr, qo.ctypes.data, 1, 1, 0, d_rows.ptr, 64, z.ctypes.data, None))
    assert ei.value.code == engine.KSP_E_LIMIT and "2^32 - 2" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_host(dbk, dbo, qk, qo, device=engine.device_count())
    assert ei.value.code == engine.KSP_E_HIP and "ksp_gather_host: no such device" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_device(**ok, device=-1)
    assert "ksp_gather_device: no such device" in str(ei.value)
    # after the refusals a valid call still succeeds, through both entries
    want = GR.gather(*case)
    got, _ = engine.gather_host(dbk, dbo, qk, qo)
    assert _tuples(got) == want
    rc, n, _ = engine.gather_device(**ok)
    assert (rc, n) == (engine.KSP_OK, len(want)) and _tuples(d_rows.to_numpy(engine.GATHER_ROW_DTYPE, n)) == want
    for b in (d_db, d_q, d_rows):
        b.free()

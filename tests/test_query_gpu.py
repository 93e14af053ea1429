"""Query mode on the GPU (kspider_amd/csrc/query.hip): ksp_query_host and ksp_query_device against brute force over
the concatenation (database runs, then query runs) filtered by the mode's rule — exact, no tolerance.  The inputs and what each
is for: tests/query_inputs.py (checked on the CPU by tests/test_query_inputs_cpu.py)."""
import numpy as np
import pytest

import query_inputs as Q
from kspider_amd import engine

pytestmark = pytest.mark.gpu
MODES = [Q.CROSS, Q.CROSS_AND_SELF]
GUARD = 64   # guard records behind an edge buffer


def _run(db_runs, q_runs, mode):
    """(edges of ksp_query_host, brute force under the mode's filter, stats, the concatenated set)"""
    sk = Q.concat(db_runs, q_runs)
    n_db = len(db_runs)
    got, st = engine.query_host(*Q.split(sk, n_db), mode=mode)
    return got, Q.expected(sk, n_db, mode), st, sk


def _same(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    assert (got == want).all()


@pytest.fixture(scope="module")
def random_case():
    db, q = Q.random_case()
    sk = Q.concat(db, q)
    return db, q, sk, {m: Q.expected(sk, len(db), m) for m in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_random_equals_brute_force_and_the_full_join(random_case, mode):
    db, q, sk, want = random_case
    got, st = engine.query_host(*Q.split(sk, len(db)), mode=mode)
    _same(got, want[mode])
    assert len(got) > 100 and st["edges"] == len(got) and st["passes"] == 1 and st["n_db"] == 260 and st["n_q"] == 40
    assert st["db_entries"] + st["q_entries"] == sk.keys.size and 0 < st["table_keys"] <= st["table_holders"] <= st["q_entries"]
    full, _ = engine.pairwise_host(sk.keys, sk.offsets)
    _same(got, Q.filter_mode(full, len(db), mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(Q.hand_made_cases()))
def test_hand_made_runs(name, mode):
    db, q = Q.hand_made_cases()[name]
    got, want, st, _ = _run(db, q, mode)
    _same(got, want)
    assert len(want) > 0 and st["edges"] == len(want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_q", [63, 64, 65, 129])
def test_query_tile(monkeypatch, n_q, mode):
    db, q = Q.tile_case(n_q)
    whole, want, st_whole, _ = _run(db, q, mode)
    monkeypatch.setenv("KSP_QUERY_TILE", "64")
    tiled, _, st, _ = _run(db, q, mode)
    _same(whole, want)
    _same(tiled, want)
    assert st_whole["passes"] == 1 and st_whole["tile"] == engine.QUERY_TILE_MAX
    assert st["passes"] == (n_q + 63) // 64 and st["tile"] == 64 and st["table_holders"] == st_whole["table_holders"]


@pytest.mark.parametrize("mode", MODES)
def test_short_and_long_kernels(monkeypatch, mode):
    db, q = Q.long_run_case()
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", "256")
    got, want, st, _ = _run(db, q, mode)
    _same(got, want)
    long_db = sum(n >= 256 for n in Q.LONG_RUN_LENGTHS)
    self_probes = len(q) - 1 if mode == Q.CROSS_AND_SELF else 0           # queries of 200 entries: short
    assert st["long_run"] == 256 and st["long_sources"] == long_db == 3 and st["short_sources"] == len(db) - long_db + self_probes
    for run in ("1", "100000"):                                            # every source long, every source short: the same rows
        monkeypatch.setenv("KSP_QUERY_LONG_RUN", run)
        other, _, st2, _ = _run(db, q, mode)
        _same(other, want)
        assert (st2["short_sources"] == 0) == (run == "1") and (st2["long_sources"] == 0) == (run != "1")


@pytest.mark.parametrize("mode", MODES)
def test_run_lengths_at_the_probe_block(monkeypatch, mode):
    """A wave looks 64 x 4 = 256 entries up per step, a workgroup 1 024: runs of 255 / 256 / 257 and 1 023 / 1 024 / 1 025 through
    the workgroup kernel (1), the three longest through it (1 000), all through the wave kernel (100 000)."""
    db, q = Q.block_case()
    sk = Q.concat(db, q)
    want = Q.expected(sk, len(db), mode)
    probes = Q.BLOCK_RUN_LENGTHS + ((Q.BLOCK_QUERY_LENGTH,) * (len(q) - 1) if mode == Q.CROSS_AND_SELF else ())
    for long_run in (1, 1000, 100000):
        monkeypatch.setenv("KSP_QUERY_LONG_RUN", str(long_run))
        got, st = engine.query_host(*Q.split(sk, len(db)), mode=mode)
        _same(got, want)
        assert st["long_run"] == long_run and st["long_sources"] == sum(n >= long_run for n in probes) and st["short_sources"] == sum(n < long_run for n in probes)
    assert sum(n >= 1000 for n in Q.BLOCK_RUN_LENGTHS) == 3 and len(want) >= len(db)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("long_run", ["1", "100000"])
@pytest.mark.parametrize("n_share", [31, 32, 33, 200])
def test_touched_list(monkeypatch, n_share, long_run, mode):
    db, q = Q.list_case(n_share)
    monkeypatch.setenv("KSP_QUERY_LIST", "32")
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", long_run)                     # the wave kernel and the workgroup kernel
    got, want, st, _ = _run(db, q, mode)
    _same(got, want)
    assert st["list_capacity"] == 32 and st["list_overflows"] == Q.expected_overflows(want, len(db), engine.QUERY_TILE_MAX, 32)
    if mode == Q.CROSS:
        assert st["list_overflows"] == (1 if n_share > 32 else 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cap", ["1", "2"])
def test_workgroup_cap(random_case, monkeypatch, cap, mode):
    db, q, sk, want = random_case
    monkeypatch.setenv("KSP_QUERY_MAX_WORKGROUPS", cap)
    sizes = np.diff(sk.offsets)[:len(db) + (len(q) - 1 if mode == Q.CROSS_AND_SELF else 0)]   # the probe sources' runs
    switch = int(np.median(sizes))
    monkeypatch.setenv("KSP_QUERY_LONG_RUN", str(switch))                  # both kernels loop over their lists
    monkeypatch.setenv("KSP_QUERY_TILE", "16")
    got, st = engine.query_host(*Q.split(sk, len(db)), mode=mode)
    _same(got, want[mode])
    assert st["long_sources"] == (sizes >= switch).sum() > 8 and st["short_sources"] == ((sizes > 0) & (sizes < switch)).sum() > 8 and st["passes"] == 3


@pytest.mark.parametrize("mode", MODES)
def test_capacity(random_case, mode):
    db, q, sk, want = random_case
    dbk, dbo, qk, qo = Q.split(sk, len(db))
    d_db, d_q = engine.DeviceBuffer.from_numpy(dbk), engine.DeviceBuffer.from_numpy(qk)
    needed = len(want[mode])
    rc, n, _ = engine.query_device(d_db.ptr, dbo, d_q.ptr, qo, None, 0, mode=mode)          # the size query
    assert (rc, n) == (engine.KSP_E_OVERFLOW, needed)
    fill = np.full((needed + GUARD) * 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for capacity in (needed - 1, needed):
        d_edges = engine.DeviceBuffer.from_numpy(fill)
        rc, n, st = engine.query_device(d_db.ptr, dbo, d_q.ptr, qo, d_edges.ptr, capacity, mode=mode)
        assert n == needed and st["edges"] == needed
        assert rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW)
        back = d_edges.to_numpy(np.uint64, fill.size)
        assert (back[2 * capacity:] == fill[2 * capacity:]).all()                            # nothing behind the capacity
        got = back[:2 * capacity].view(engine.EDGE_DTYPE)
        got = got[np.lexsort((got["source_2"], got["source_1"]))]                            # the order is unspecified
        if capacity == needed:
            _same(got, want[mode])
        else:                                                                                # all but one of the rows, each once
            rows = {tuple(r) for r in want[mode].tolist()}
            assert len({tuple(r) for r in got.tolist()}) == capacity and all(tuple(r) in rows for r in got.tolist())
        d_edges.free()
    d_db.free()
    d_q.free()


def test_refusals_and_a_valid_call_after_them(monkeypatch):
    db, q = Q.hand_made_cases()["one_hash_sources"]
    sk = Q.concat(db, q)
    dbk, dbo, qk, qo = Q.split(sk, len(db))
    d_db, d_q, d_edges = engine.DeviceBuffer.from_numpy(dbk), engine.DeviceBuffer.from_numpy(qk), engine.DeviceBuffer(16 * 64)
    z = np.zeros(1, np.uint64)
    arg_cases = [(None, dbo, d_q.ptr, qo, d_edges.ptr, 64, 0), (d_db.ptr, None, d_q.ptr, qo, d_edges.ptr, 64, 0), (d_db.ptr, dbo, None, qo, d_edges.ptr, 64, 0),
                 (d_db.ptr, dbo, d_q.ptr, None, d_edges.ptr, 64, 0), (d_db.ptr, dbo, d_q.ptr, qo, None, 64, 0),
                 (d_db.ptr, z, d_q.ptr, qo, d_edges.ptr, 64, 0), (d_db.ptr, dbo, d_q.ptr, z, d_edges.ptr, 64, 0),
                 (d_db.ptr, dbo + 1, d_q.ptr, qo, d_edges.ptr, 64, 0), (d_db.ptr, dbo, d_q.ptr, qo[::-1].copy(), d_edges.ptr, 64, 0),
                 (d_db.ptr, dbo, d_q.ptr, qo, d_edges.ptr, 64, 2), (d_db.ptr, dbo, d_q.ptr, qo, d_edges.ptr, 64, -1)]
    for *args, mode in arg_cases:
        with pytest.raises(engine.KspError) as ei:
            engine.query_device(*args, mode=mode)
        assert ei.value.code == engine.KSP_E_ARG, args
    with pytest.raises(engine.KspError) as ei:                             # n_edges itself NULL
        engine._check(engine.lib().ksp_query_device(0, d_db.ptr, dbo.ctypes.data, len(db), d_q.ptr, qo.ctypes.data, len(q), 0, d_edges.ptr, 64, None, None))
    assert ei.value.code == engine.KSP_E_ARG
    for name, value in [("KSP_QUERY_TILE", "0"), ("KSP_QUERY_TILE", str(engine.QUERY_TILE_MAX + 1)), ("KSP_QUERY_LIST", "0"),
                        ("KSP_QUERY_LIST", str(engine.QUERY_LIST_MAX + 1)), ("KSP_QUERY_LONG_RUN", "many")]:
        monkeypatch.setenv(name, value)
        with pytest.raises(engine.KspError) as ei:
            engine.query_host(dbk, dbo, qk, qo)
        assert ei.value.code == engine.KSP_E_ARG and name in str(ei.value)
        monkeypatch.delenv(name)
    # KSP_E_LIMIT: a query tile of 2^31 entries (the offsets say so; no key of it is read), and memory that cannot fit
    huge = np.array([0, 2**31], dtype=np.uint64)
    with pytest.raises(engine.KspError) as ei:
        engine.query_device(d_db.ptr, dbo, d_q.ptr, huge, d_edges.ptr, 64)
    assert ei.value.code == engine.KSP_E_LIMIT and "2^31" in str(ei.value)
    claims = np.array([0, 2**40], dtype=np.uint64)                         # 8 TiB of database keys: refused from the offsets, no key is read
    with pytest.raises(engine.KspError) as ei:
        engine.query_host(dbk, claims, qk, qo)
    assert ei.value.code == engine.KSP_E_LIMIT and "bytes of device memory" in str(ei.value) and "are free" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:                             # 2^32 - 1 sources, from the counts alone: no offset of them is read
        engine._check(engine.lib().ksp_query_device(0, d_db.ptr, dbo.ctypes.data, 2**32 - 2, d_q.ptr, qo.ctypes.data, 1, 0, d_edges.ptr, 64, z.ctypes.data, None))
    assert ei.value.code == engine.KSP_E_LIMIT and "2^32 - 2" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.query_host(dbk, dbo, qk, qo, device=engine.device_count())
    assert ei.value.code == engine.KSP_E_HIP and "ksp_query_host: no such device" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.query_device(d_db.ptr, dbo, d_q.ptr, qo, d_edges.ptr, 64, device=-1)
    assert "ksp_query_device: no such device" in str(ei.value)
    # after the refusals a valid call still succeeds, through both entries
    for mode in MODES:
        want = Q.expected(sk, len(db), mode)
        got, _ = engine.query_host(dbk, dbo, qk, qo, mode=mode)
        _same(got, want)
        rc, n, _ = engine.query_device(d_db.ptr, dbo, d_q.ptr, qo, d_edges.ptr, 64, mode=mode)
        assert (rc, n) == (engine.KSP_OK, len(want))
        got = d_edges.to_numpy(engine.EDGE_DTYPE, n)
        _same(got[np.lexsort((got["source_2"], got["source_1"]))], want)
    for b in (d_db, d_q, d_edges):
        b.free()

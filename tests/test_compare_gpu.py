"""Compare on the GPU (kspider_amd/csrc/compare.hip): ksp_compare_host and ksp_compare_device against the
restatement (tests/compare_restate.py) — integers, so equal, not close.  The inputs and what each is for: tests/compare_inputs.py
(checked on the CPU by tests/test_compare_inputs_cpu.py)."""
import numpy as np
import pytest

import compare_inputs as C
import compare_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu
MODES = [R.CROSS, R.CROSS_AND_SELF]
GUARD = 64   # guard words behind a row buffer


def _want(db, q, mode):
    rows = np.array(R.rows(db, q, mode), dtype=engine.WEDGE_DTYPE).reshape(-1)
    total, sq = R.totals(list(db) + list(q))
    return rows, np.array(total, dtype=np.uint64), np.array(sq, dtype=np.uint64)


def _run(db, q, mode, db_counted=True, q_counted=True):
    """(rows, sum, sumsq, stats) of ksp_compare_host; a database of no source goes in as three NULLs"""
    side = C.arrays(db, db_counted) if db else (None, None, None)
    return engine.compare_host(*side, *C.arrays(q, q_counted), mode=mode)


def _same(got, want):
    rows, total, sq = want
    assert got[0].dtype == rows.dtype and len(got[0]) == len(rows), (len(got[0]), len(rows))
    assert (got[0] == rows).all() and (got[1] == total).all() and (got[2] == sq).all()


def test_hand_case():
    db, q = C.hand_case()
    got = _run(db, q, R.CROSS_AND_SELF)
    assert [tuple(r) for r in got[0].tolist()] == C.HAND_ROWS and (got[1].tolist(), got[2].tolist()) == C.HAND_SUMS
    assert 4 not in got[0]["source_1"] and 4 not in got[0]["source_2"]          # the disjoint sample has no row
    same = got[0][3]                                                            # q0 and q1 are one sample: exactly 1
    assert engine.compare_values(same, 3, 8, 26, 3, 8, 26) == (1.0, 1.0, 1.0, 1.0)
    _same(_run(db, q, R.CROSS), _want(db, q, R.CROSS))
    _same(_run([], db + q, R.CROSS_AND_SELF), _want([], db + q, R.CROSS_AND_SELF))
    # a flat database against counted samples, through the NULL pointer and through an array of ones
    _same(_run(db, q, R.CROSS_AND_SELF, db_counted=False), _want(C.flat(db), q, R.CROSS_AND_SELF))
    _same(_run(C.flat(db), q, R.CROSS_AND_SELF), _want(C.flat(db), q, R.CROSS_AND_SELF))


@pytest.fixture(scope="module")
def random_case():
    db, q = C.random_case()
    return db, q, {m: _want(db, q, m) for m in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_random_equals_the_restatement(random_case, mode):
    db, q, want = random_case
    got = _run(db, q, mode)
    _same(got, want[mode])
    st = got[3]
    assert st["edges"] == len(got[0]) > 100 and st["passes"] == 1 and (st["n_db"], st["n_q"]) == (12, 28) and st["tile"] == engine.COMPARE_TILE_MAX
    assert st["db_entries"] + st["q_entries"] == sum(len(s) for s in db + q) and 0 < st["table_keys"] <= st["table_holders"] == st["q_entries"]
    # one side counted only: the other's NULL pointer stands for ones
    _same(_run(db, q, mode, db_counted=False), _want(C.flat(db), q, mode))
    _same(_run(db, q, mode, q_counted=False), _want(db, C.flat(q), mode))


def test_random_without_a_database(random_case):
    db, q, _ = random_case
    _same(_run([], db + q, R.CROSS_AND_SELF), _want([], db + q, R.CROSS_AND_SELF))


@pytest.mark.parametrize("mode", MODES)
def test_flat_sketches_give_query_mode_s_counts(random_case, mode):
    db, q, _ = random_case
    got = _run(db, q, mode, db_counted=False, q_counted=False)
    dk, _, do = C.arrays(db)
    qk, _, qo = C.arrays(q)
    edges, _ = engine.query_host(dk, do, qk, qo, mode=mode)
    rows = got[0]
    assert len(rows) == len(edges) and all((rows[f] == edges[f]).all() for f in ("source_1", "source_2", "shared"))
    assert all((rows[f] == rows["shared"]).all() for f in ("dot", "mass_1", "mass_2"))
    assert (got[1] == got[2]).all() and got[1].tolist() == [len(s) for s in db + q]


def test_width():
    db, q = C.width_case()
    got = _run(db, q, R.CROSS_AND_SELF)
    _same(got, _want(db, q, R.CROSS_AND_SELF))
    assert int(got[0]["dot"][0]) == 2**64 - 2**33 + 1 and int(got[0]["dot"][1]) == 120 * 2**30


@pytest.mark.parametrize("side", ["database", "query"])
def test_the_refusal_at_its_exact_value(side):
    for last, refused in ((2, False), (3, True)):
        big, small = C.limit_case(last)
        db, q = ([big], [small]) if side == "database" else ([small], [small, big])
        if not refused:
            got = _run(db, q, R.CROSS_AND_SELF)
            _same(got, _want(db, q, R.CROSS_AND_SELF))
            assert 2**64 - 1 in [int(v) for v in got[2]]
            continue
        with pytest.raises(engine.KspError) as ei:
            _run(db, q, R.CROSS_AND_SELF)
        assert ei.value.code == engine.KSP_E_LIMIT and ("database source 0" if side == "database" else "query source 1") in str(ei.value) and "2^64" in str(ei.value)


@pytest.fixture(scope="module")
def seams():
    db, q = C.seams_case()
    return q, C.arrays(q), _want(db, q, R.CROSS_AND_SELF)


@pytest.mark.parametrize("tile", [None, "1", "3"])
def test_seams(seams, monkeypatch, tile):
    q, side, want = seams
    if tile:
        monkeypatch.setenv("KSP_COMPARE_TILE", tile)
    got = engine.compare_host(None, None, None, *side, mode=R.CROSS_AND_SELF)
    _same(got, want)
    assert got[3]["tile"] == int(tile or engine.COMPARE_TILE_MAX) and got[3]["passes"] == -(-1100 // got[3]["tile"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,value", [("KSP_COMPARE_LONG_RUN", "1"), ("KSP_COMPARE_LONG_RUN", "150"), ("KSP_COMPARE_MAX_WORKGROUPS", "1"),
                                        ("KSP_COMPARE_MAX_WORKGROUPS", "3"), ("KSP_COMPARE_TILE", "5")])
def test_switches_on_the_random_case(random_case, monkeypatch, name, value, mode):
    db, q, want = random_case
    monkeypatch.setenv(name, value)
    if name == "KSP_COMPARE_MAX_WORKGROUPS":
        monkeypatch.setenv("KSP_COMPARE_LONG_RUN", "150")                       # both kernels, and every group of each loops
        monkeypatch.setenv("KSP_COMPARE_TILE", "16")
    got = _run(db, q, mode)
    _same(got, want[mode])
    st = got[3]
    probes = [len(s) for s in db] + ([len(s) for s in q[:-1]] if mode == R.CROSS_AND_SELF else [])
    long_run = 150 if name == "KSP_COMPARE_MAX_WORKGROUPS" else int(value) if name == "KSP_COMPARE_LONG_RUN" else engine.QUERY_LONG_RUN
    assert st["long_sources"] == sum(n >= long_run for n in probes) and st["short_sources"] == sum(n < long_run for n in probes)
    if name == "KSP_COMPARE_LONG_RUN":
        assert (st["short_sources"] == 0) == (value == "1") and st["long_sources"] > 0
    if name == "KSP_COMPARE_MAX_WORKGROUPS":                                    # a workgroup is one long group or four short ones
        assert st["passes"] == 2 and st["long_sources"] > int(value) and (mode == R.CROSS or st["short_sources"] > 4 * int(value))


@pytest.mark.parametrize("long_run", [None, "1"])
@pytest.mark.parametrize("cap", ["1", "4", None])
def test_touched_list(monkeypatch, cap, long_run):
    db, q = C.list_case()
    if cap:
        monkeypatch.setenv("KSP_COMPARE_LIST", cap)
    if long_run:
        monkeypatch.setenv("KSP_COMPARE_LONG_RUN", long_run)
    got = _run(db, q, R.CROSS_AND_SELF)
    _same(got, _want(db, q, R.CROSS_AND_SELF))
    limit = int(cap or engine.COMPARE_LIST_MAX)
    assert got[3]["list_capacity"] == limit and got[3]["list_overflows"] == sum(299 - s > limit for s in range(299)) > 0


def test_capacity_and_the_retry(random_case, monkeypatch):
    db, q, want = random_case
    rows = want[R.CROSS_AND_SELF][0]
    needed = len(rows)
    dk, da, do = C.arrays(db)
    qk, qa, qo = C.arrays(q)
    bufs = [engine.DeviceBuffer.from_numpy(a) for a in (dk, da, qk, qa)]
    ptrs = (bufs[0].ptr, bufs[1].ptr, do, bufs[2].ptr, bufs[3].ptr, qo)
    rc, n, total, sq, _ = engine.compare_device(*ptrs, None, 0)                 # the size query
    assert (rc, n) == (engine.KSP_E_OVERFLOW, needed) and (total == want[R.CROSS_AND_SELF][1]).all() and (sq == want[R.CROSS_AND_SELF][2]).all()
    fill = np.full((needed + GUARD) * 5, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for capacity in (needed - 1, needed):
        d_rows = engine.DeviceBuffer.from_numpy(fill)
        rc, n, _, _, st = engine.compare_device(*ptrs, d_rows.ptr, capacity)
        assert n == needed == st["edges"] and rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW)
        back = d_rows.to_numpy(np.uint64, fill.size)
        assert (back[5 * capacity:] == fill[5 * capacity:]).all()               # nothing behind the capacity
        got = back[:5 * capacity].view(engine.WEDGE_DTYPE)
        got = got[np.lexsort((got["source_2"], got["source_1"]))]               # the order is unspecified
        if capacity == needed:
            assert (got == rows).all()
        else:                                                                   # all but one of the rows, each once
            known = {tuple(r) for r in rows.tolist()}
            assert len({tuple(r) for r in got.tolist()}) == capacity and all(tuple(r) in known for r in got.tolist())
        d_rows.free()
    for b in bufs:
        b.free()
    # the host call: a first buffer one row short, then the exact size
    monkeypatch.setenv("KSP_COMPARE_FIRST_CAPACITY", str(needed - 1))
    _same(_run(db, q, R.CROSS_AND_SELF), want[R.CROSS_AND_SELF])
    monkeypatch.setenv("KSP_COMPARE_FIRST_CAPACITY", "1")
    _same(_run(db, q, R.CROSS), want[R.CROSS])


def test_refusals_on_the_device_and_a_valid_call_after_them(monkeypatch):
    db, q = C.hand_case()
    want = _want(db, q, R.CROSS_AND_SELF)
    dk, da, do = C.arrays(db)
    qk, qa, qo = C.arrays(q)

    def refused(code, text, **changed):
        args = dict(dk=dk, da=da, do=do, qk=qk, qa=qa, qo=qo)
        args.update(changed)
        with pytest.raises(engine.KspError) as ei:
            engine.compare_host(args["dk"], args["da"], args["do"], args["qk"], args["qa"], args["qo"], mode=R.CROSS_AND_SELF)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    repeated, descending, zero = qk.copy(), qk.copy(), qa.copy()
    repeated[4] = repeated[3]                                                   # q1 = entries 3 .. 5
    descending[7], descending[8] = qk[8], qk[7]                                 # q2 = entries 6 .. 8
    zero[10] = 0                                                                # q3 = entries 9, 10
    refused(engine.KSP_E_ARG, "query source 1 is not strictly ascending", qk=repeated)
    refused(engine.KSP_E_ARG, "query source 2 is not strictly ascending", qk=descending)
    refused(engine.KSP_E_ARG, "query source 3 has an abundance of 0", qa=zero)
    refused(engine.KSP_E_ARG, "database source 0 is not strictly ascending", dk=dk[::-1].copy())
    refused(engine.KSP_E_ARG, "database source 0 has an abundance of 0", da=np.zeros_like(da))
    for name, value in [("KSP_COMPARE_TILE", "0"), ("KSP_COMPARE_TILE", str(engine.COMPARE_TILE_MAX + 1)), ("KSP_COMPARE_LIST", "0"),
                        ("KSP_COMPARE_LIST", str(engine.COMPARE_LIST_MAX + 1)), ("KSP_COMPARE_LONG_RUN", "many")]:
        monkeypatch.setenv(name, value)
        refused(engine.KSP_E_ARG, name)
        monkeypatch.delenv(name)
    refused(engine.KSP_E_LIMIT, "bytes of device memory", do=np.array([0, 2**40], dtype=np.uint64))   # refused from the offsets: no key is read
    with pytest.raises(engine.KspError) as ei:
        engine.compare_host(dk, da, do, qk, qa, qo, device=engine.device_count())
    assert ei.value.code == engine.KSP_E_HIP and "ksp_compare_host: no such device" in str(ei.value)
    _same(_run(db, q, R.CROSS_AND_SELF), want)

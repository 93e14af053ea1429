"""Compare's kernels (kspider_amd/csrc/compare.hip) where tests/test_compare_gpu.py does not reach: the probe's entry
loop beyond its first trip, the lane-local carry of the totals, sums other than dot across the 32-bit word, the check at the seam
between two trips and with several faulty sources, empty sources and sides, a full tile, keys 0 and 2^64 - 1 and a table of one
bucket.  Every assertion is equality with the restatement (tests/compare_restate.py); the inputs are tests/compare_inputs.py, each
shown on the CPU to be the case it is named for (tests/test_compare_inputs_cpu.py)."""
import numpy as np
import pytest

import compare_inputs as C
import compare_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu
MODES = [R.CROSS, R.CROSS_AND_SELF]
KERNELS = {"wave": "100000", "workgroup": "1"}   # KSP_COMPARE_LONG_RUN: every probe source through one kernel


def _want(db, q, mode):
    rows = np.array(R.rows(db, q, mode), dtype=engine.WEDGE_DTYPE).reshape(-1)
    total, sq = R.totals(list(db) + list(q))
    return rows, np.array(total, dtype=np.uint64), np.array(sq, dtype=np.uint64)


def _run(db, q, mode):
    """(rows, sum, sumsq, stats) of ksp_compare_host; a database of no source goes in as three NULLs"""
    side = C.arrays(db) if db else (None, None, None)
    return engine.compare_host(*side, *C.arrays(q), mode=mode)


def _same(got, want):
    rows, total, sq = want
    assert got[0].dtype == rows.dtype and len(got[0]) == len(rows), (len(got[0]), len(rows))
    assert (got[0] == rows).all() and (got[1] == total).all() and (got[2] == sq).all()


def _refused(db_side, q_side, code, text, mode=R.CROSS_AND_SELF):
    with pytest.raises(engine.KspError) as ei:
        engine.compare_host(*db_side, *q_side, mode=mode)
    assert ei.value.code == code and text in str(ei.value), str(ei.value)


# ---- the probe's entry loop --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block():
    db, q = C.block_case()
    return db, q, {m: _want(db, q, m) for m in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("long_run", [1, 1000, 100000])
def test_run_lengths_at_the_probe_s_trips(block, monkeypatch, long_run, mode):
    """A wave looks 64 x 4 = 256 entries up per trip, a workgroup 1 024: runs of 255 / 256 / 257 and 1 023 / 1 024 / 1 025 through
    the workgroup kernel (1), the three longest through it (1 000), all through the wave kernel (100 000)."""
    db, q, want = block
    monkeypatch.setenv("KSP_COMPARE_LONG_RUN", str(long_run))
    got = _run(db, q, mode)
    _same(got, want[mode])
    probes = C.BLOCK_RUN_LENGTHS + ((C.BLOCK_QUERY_LENGTH,) * (len(q) - 1) if mode == R.CROSS_AND_SELF else ())
    st = got[3]
    assert st["long_run"] == long_run and st["long_sources"] == sum(n >= long_run for n in probes) and st["short_sources"] == sum(n < long_run for n in probes)
    assert sum(n >= 1000 for n in C.BLOCK_RUN_LENGTHS) == 3 and len(got[0]) >= 6 * 12


# ---- the totals: a carry inside one lane ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["database", "query"])
def test_a_carry_inside_one_lane_of_the_totals(side):
    for accepted in (True, False):
        big, small = C.lane_carry_case(accepted)
        db, q = ([small, big], [small]) if side == "database" else ([small], [small, small, big])
        if accepted:
            got = _run(db, q, R.CROSS_AND_SELF)
            _same(got, _want(db, q, R.CROSS_AND_SELF))
            assert [int(v) for v in got[2]].count(2**64 - 1) == 1
        else:
            name = "database source 1" if side == "database" else "query source 2"
            _refused(C.arrays(db), C.arrays(q), engine.KSP_E_LIMIT, "the squared abundances of " + name + " sum to 2^64 or more")


@pytest.mark.parametrize("workgroups", [None, "1"])
def test_the_smallest_carrying_source_is_named(monkeypatch, workgroups):
    if workgroups:
        monkeypatch.setenv("KSP_COMPARE_MAX_WORKGROUPS", workgroups)
    db, q = C.lane_carry_many()
    _refused(C.arrays(db), C.arrays(q), engine.KSP_E_LIMIT, "the squared abundances of database source 1 sum")
    _refused(C.arrays(db), C.arrays(q), engine.KSP_E_LIMIT, "the squared abundances of database source 1 sum", mode=R.CROSS)
    _refused((None, None, None), C.arrays(q[1:]), engine.KSP_E_LIMIT, "the squared abundances of query source 1 sum")
    _refused(C.arrays(db[:1] + db[2:3]), C.arrays(q), engine.KSP_E_LIMIT, "the squared abundances of query source 0 sum")
    good = (db[:1] + db[2:3], q[1:2] + q[3:])
    _same(_run(*good, R.CROSS_AND_SELF), _want(*good, R.CROSS_AND_SELF))


# ---- every 64-bit sum across the word ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mass_width():
    first, second = C.mass_width_case()
    return {name: (db, q, _want(db, q, R.CROSS_AND_SELF)) for name, (db, q) in {"database": ([first], [second]), "queries": ([], [first, second])}.items()}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("sides", ["database", "queries"])
def test_masses_and_sums_of_2_32_and_more(mass_width, monkeypatch, sides, kernel):
    db, q, want = mass_width[sides]
    monkeypatch.setenv("KSP_COMPARE_LONG_RUN", KERNELS[kernel])
    got = _run(db, q, R.CROSS_AND_SELF)
    _same(got, want)
    (row,) = got[0]
    assert min(int(row["dot"]), int(row["mass_1"]), int(row["mass_2"]), int(got[1].min())) >= 2**32 and int(row["shared"]) == C.MASS_N
    assert (got[3]["long_sources"], got[3]["short_sources"]) == ((1, 0) if kernel == "workgroup" else (0, 1))


# ---- the check at its seams ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seams():
    db, q = C.check_seams_base()
    return db, q, _want(db, q, R.CROSS_AND_SELF), C.check_seams_variants()


@pytest.mark.parametrize("workgroups", [None, "1"])
@pytest.mark.parametrize("name", ["equal_at_255_256", "descending_at_255_256", "zero_at_256", "zero_at_the_last_entry", "bad_runs_on_both_sides",
                                  "bad_runs_in_the_queries", "zeros_on_both_sides", "order_fault_behind_a_zero"])
def test_the_check_names_the_fault(seams, monkeypatch, name, workgroups):
    """One workgroup reads a source 256 entries per trip; with KSP_COMPARE_MAX_WORKGROUPS=1 the same workgroup reads every source,
    one after the other.  An order fault is reported before an abundance of 0, whichever source is the smaller."""
    db, q, want, variants = seams
    if workgroups:
        monkeypatch.setenv("KSP_COMPARE_MAX_WORKGROUPS", workgroups)
    db_side, q_side, message = variants[name]
    _refused(db_side, q_side, engine.KSP_E_ARG, message)
    _same(_run(db, q, R.CROSS_AND_SELF), want)                                   # (the base: a run may end above the next one's first key, or at it)


# ---- empty sources ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,value,passes", [(None, None, 1), ("KSP_COMPARE_TILE", "2", 2), ("KSP_COMPARE_TILE", "1", 3), ("KSP_COMPARE_LONG_RUN", "1", 1)])
def test_empty_sources(monkeypatch, name, value, passes, mode):
    db, q = C.empties_case()
    if name:
        monkeypatch.setenv(name, value)
    got = _run(db, q, mode)
    _same(got, _want(db, q, mode))
    empty = [s for s, src in enumerate(db + q) if not src]
    assert len(got[0]) > 0 and not (np.isin(got[0]["source_1"], empty) | np.isin(got[0]["source_2"], empty)).any()
    assert (got[1][empty] == 0).all() and (got[2][empty] == 0).all() and got[3]["passes"] == passes      # a tile without an entry is no pass
    probes = [len(s) for s in db] + ([len(s) for s in q[:-1]] if mode == R.CROSS_AND_SELF else [])
    assert got[3]["long_sources"] + got[3]["short_sources"] == sum(n > 0 for n in probes)               # an empty source does not probe


@pytest.mark.parametrize("mode", MODES)
def test_empty_sides(mode):
    """A database of empty sources; queries that are all empty (no tile has an entry, so no table is built): the rows of the mode
    that remain, none where nothing can share, and the totals of every source, KSP_OK."""
    db, q = C.empties_case()
    for sides in (([{}, {}, {}], q), (db, [{}] * 6), ([{}, {}], [{}]), ([], [{}, {}]) if mode == R.CROSS_AND_SELF else ([{}], [{}, {}])):
        got = _run(*sides, mode)
        want = _want(*sides, mode)
        _same(got, want)
        assert len(got[0]) == (6 - 3 if mode == R.CROSS_AND_SELF and any(sides[1]) else 0) and got[3]["edges"] == len(got[0])
        if not any(sides[1]):
            assert got[3]["passes"] == 0 and got[3]["table_keys"] == 0
    _same(_run(db, q, mode), _want(db, q, mode))


# ---- a full tile -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_tile():
    db, q = C.full_tile_case()
    return C.arrays(q), _want(db, q, R.CROSS_AND_SELF)


@pytest.mark.parametrize("long_run", [None, "1"])
def test_a_full_tile_and_one_query_more(full_tile, monkeypatch, long_run):
    side, want = full_tile
    if long_run:
        monkeypatch.setenv("KSP_COMPARE_LONG_RUN", long_run)
    got = engine.compare_host(None, None, None, *side, mode=R.CROSS_AND_SELF)
    _same(got, want)
    st = got[3]
    assert len(got[0]) == 131328 and st["passes"] == 2 and st["tile"] == 512 and (st["long_sources"] == 512) == bool(long_run)
    assert st["list_overflows"] == C.expected_overflows(want[0].tolist(), 0, 512, engine.COMPARE_LIST_MAX) == 255


# ---- extreme and clustered keys ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", [None, "1"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["ends", "one_bucket", "only_zero"])
def test_extreme_keys(monkeypatch, name, kernel, tile, mode):
    db, q = C.extreme_keys_cases()[name]
    monkeypatch.setenv("KSP_COMPARE_LONG_RUN", KERNELS[kernel])
    if tile:
        monkeypatch.setenv("KSP_COMPARE_TILE", tile)
    got = _run(db, q, mode)
    _same(got, _want(db, q, mode))
    assert len(got[0]) > 0 and got[3]["passes"] == (len(q) if tile else 1)
    if mode == R.CROSS_AND_SELF:                                                 # the same sources as queries only: the holders' side has them all
        _same(_run([], db + q, mode), _want([], db + q, mode))

"""Weighted gather on the GPU (kspider_amd/csrc/gather.hip): ksp_gather_abund_host and ksp_gather_abund_device
against the restatement in Python ints (tests/gather_abund_restate.py) — exact, compared with ==.  The inputs and what each is
for: tests/gather_abund_inputs.py (checked on the CPU, against rows written out by hand, by tests/test_gather_abund_inputs_cpu.py)."""
import functools

import numpy as np
import pytest

import gather_abund_inputs as I
import gather_abund_restate as WR
from kspider_amd import engine

pytestmark = pytest.mark.gpu
GUARD = 8   # guard rows behind a row buffer
MASK = 2**64 - 1


def _tuples(rows):
    """the rows as the restatement writes them: the two words of the sum of squares joined"""
    return [tuple(int(r[n]) for n in ("query", "rank", "source", "overlap", "unique", "remaining", "w_unique", "w_found")) + ((int(r["sq_hi"]) << 64) | int(r["sq_lo"]), int(r["median2"]))
            for r in rows]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, the restatement's rows), made once"""
    if name in I.hand_made_cases():
        case = I.hand_made_cases()[name]
    else:
        case = {"sizes": I.sizes_case, "digits_small": lambda: I.digit_case(1), "digits_large": lambda: I.digit_case(40), "equal": I.equal_case, "dead_part": I.dead_part_case,
                "tiles": I.tiles_case, "tiles_ones": lambda: I.ones(I.tiles_case()), "sizes_ones": lambda: I.ones(I.sizes_case())}[name]()
    return case, WR.gather(*case)


def _run(case):
    db, q, a, m, k = case
    dk, do, qk, qa, qo = I.arrays(db, q, a)
    got, st = engine.gather_abund_host(dk, do, qk, qa, qo, min_hashes=m, max_matches=k)
    plain, _ = engine.gather_host(dk, do, qk, qo, min_hashes=m, max_matches=k)
    assert [r[:6] for r in _tuples(got)] == [tuple(int(v) for v in r) for r in plain.tolist()]      # the first six fields are the unweighted call's
    return _tuples(got), st


@pytest.mark.parametrize("name", sorted(I.hand_made_cases()))
def test_hand_made(name):
    case, want = _case(name)
    got, st = _run(case)
    assert got == want and st["rows"] == len(want)


@pytest.mark.parametrize("name", ["sizes", "digits_small", "digits_large", "equal", "dead_part", "tiles"])
def test_against_the_restatement(name):
    """Taken sets of 1, 2, 63, 64, 65, 1 023, 1 024 and 1 025 hashes; middle values on both sides of every digit boundary, ranked in
    registers and selected by digits; all values equal, 0 and 2^32 - 1 (the upper word of the sum of squares); a segment that is
    partly dead; queries of one tile that hold the same hashes with other abundances."""
    case, want = _case(name)
    got, _ = _run(case)
    assert got == want
    if name == "equal":
        assert got[1][8] >> 64 > 0


@pytest.mark.parametrize("name", ["tiles_ones", "sizes_ones"])
def test_all_abundances_one(name):
    case, want = _case(name)
    got, _ = _run(case)
    assert got == want
    for r in got:
        assert r[6] == r[4] == r[8] and r[9] == 2


SWITCHES = [{"KSP_QUERY_TILE": "1"}, {"KSP_QUERY_TILE": "2", "KSP_GATHER_TAIL": "0"}, {"KSP_GATHER_TAIL": "0"}, {"KSP_GATHER_TAIL": "1", "KSP_GATHER_TAIL_CANDS": "1048576"},
            {"KSP_GATHER_MAX_WORKGROUPS": "1"}, {"KSP_GATHER_MAX_WORKGROUPS": "1", "KSP_GATHER_TAIL": "0", "KSP_GATHER_LONG_SEG": "4"},
            {"KSP_GATHER_TAIL_CANDS": "0"}, {"KSP_QUERY_TILE": "3", "KSP_QUERY_LIST": "1", "KSP_QUERY_LONG_RUN": "8"}]


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "-".join(f"{k[4:]}={v}" for k, v in s.items()))
def test_the_rows_are_the_same_under_every_switch(monkeypatch, switches):
    """Tiles of one, two and three queries (the abundances are looked up per tile), rounds in batches to the end and in the
    one-workgroup tail from the first round on, one workgroup for everything"""
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    for name in ("tiles", "sizes", "digits_large", "dead_part", "same_hash_two_queries"):
        case, want = _case(name)
        got, st = _run(case)
        assert got == want, name
        if switches.get("KSP_GATHER_TAIL") == "0":
            assert st["tail_rounds"] == 0
        if "KSP_GATHER_TAIL_CANDS" in switches and switches["KSP_GATHER_TAIL_CANDS"] != "0":
            assert st["tail_rounds"] == st["rounds"] > 0


def test_device_entry_size_query_and_row_overflow():
    case, want = _case("tiles")
    dk, do, qk, qa, qo = I.arrays(*case[:3])
    d_db, d_q, d_a = engine.DeviceBuffer.from_numpy(dk), engine.DeviceBuffer.from_numpy(qk), engine.DeviceBuffer.from_numpy(qa)
    needed = len(want)
    rc, n, _ = engine.gather_abund_device(d_db.ptr, do, d_q.ptr, d_a.ptr, qo, None, 0, min_hashes=case[3])      # the size query
    assert (rc, n) == (engine.KSP_E_OVERFLOW, needed)
    fill = np.full((needed + GUARD) * 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for capacity in (needed - 1, needed):
        d_rows = engine.DeviceBuffer.from_numpy(fill)
        rc, n, st = engine.gather_abund_device(d_db.ptr, do, d_q.ptr, d_a.ptr, qo, d_rows.ptr, capacity, min_hashes=case[3])
        assert n == needed and st["rows"] == needed and rc == (engine.KSP_OK if capacity == needed else engine.KSP_E_OVERFLOW)
        back = d_rows.to_numpy(np.uint64, fill.size)
        assert (back[8 * capacity:] == fill[8 * capacity:]).all()                                    # nothing behind the capacity
        assert _tuples(back[:8 * capacity].view(engine.GATHER_WROW_DTYPE)) == want[:capacity]         # the first rows, in order
        d_rows.free()
    # refusals of the weighted entries: the abundances missing, rows missing with a capacity
    for change, text in ((dict(d_q_abund_ptr=None), "NULL argument"), (dict(d_rows_ptr=None, capacity=4), "d_rows is NULL but capacity is not 0")):
        args = dict(d_db_keys_ptr=d_db.ptr, db_offsets=do, d_q_keys_ptr=d_q.ptr, d_q_abund_ptr=d_a.ptr, q_offsets=qo, d_rows_ptr=None, capacity=0)
        with pytest.raises(engine.KspError) as ei:
            engine.gather_abund_device(**{**args, **change}, device=99)
        assert ei.value.code == engine.KSP_E_ARG and f"ksp_gather_abund_device: {text}" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_abund_host(dk, do, qk, qa, qo, device=engine.device_count())
    assert ei.value.code == engine.KSP_E_HIP and "ksp_gather_abund_host: no such device" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_abund_host(dk, np.array([0, 2**40], dtype=np.uint64), qk, qa, qo)
    assert ei.value.code == engine.KSP_E_LIMIT and "bytes of device memory" in str(ei.value)
    for b in (d_db, d_q, d_a):
        b.free()

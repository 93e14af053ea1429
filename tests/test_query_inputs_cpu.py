"""The builders of tests/query_inputs.py make the cases they are named for, and the host-only parts of query mode (the
directory's bits and shift, the symbols, the refusals that need no device) behave as include/kspider_amd.h says."""
import ctypes

import numpy as np
import pytest

import oracle
import query_inputs as Q
from kspider_amd import engine


def _table_keys(q_runs):
    return np.unique(np.concatenate([np.asarray(list(r), dtype=np.uint64) for r in q_runs]))


def test_directory_bits_and_shift():
    assert engine.query_directory(0, 1) == (0, 0)
    assert engine.query_directory(1, 1) == (1, 0)
    assert engine.query_directory(Q.TOP, 2) == (1, 63)            # never a shift of 64
    assert engine.query_directory(Q.TOP, 4 << 10) == (10, 54)     # four keys per bucket
    assert engine.query_directory(Q.TOP, (4 << 10) + 1) == (11, 53)
    assert engine.query_directory(255, 10**6) == (8, 0)           # not more bits than the key has
    assert engine.query_directory(Q.TOP, 10**12) == (engine.QUERY_DIR_BITS_MAX, 64 - engine.QUERY_DIR_BITS_MAX)
    for max_key, n in [(5, 3), (2**40 + 126, 64), (2**63, 500000)]:
        bits, shift = engine.query_directory(max_key, n)
        assert bits + shift == int(max_key).bit_length() and (max_key >> shift) < (1 << bits)


def test_one_bucket_case_is_one_bucket():
    db_runs, q_runs = Q.one_bucket_case()
    tk = _table_keys(q_runs)
    assert tk.size == 64
    bits, shift = engine.query_directory(int(tk.max()), tk.size)
    assert bits >= 1 and len({int(k) >> shift for k in tk}) == 1   # 2^bits buckets, all keys in one of them
    bucket = int(tk[0]) >> shift
    db = np.unique(np.concatenate([np.asarray(r, dtype=np.uint64) for r in db_runs]))
    in_bucket = [int(k) for k in db if int(k) >> shift == bucket]
    table = {int(k) for k in tk}
    assert any(k in table for k in in_bucket)                                  # hits
    assert any(k not in table and k < int(tk.max()) for k in in_bucket)        # misses that search the bucket
    assert any(k > int(tk.max()) for k in in_bucket)                           # a miss above the largest key
    assert any(int(k) >> shift != bucket for k in db)                          # and keys of other buckets


def test_hand_made_cases_hold_what_they_name():
    cases = Q.hand_made_cases()
    db, q = cases["empty_query"]
    assert any(len(r) == 0 for r in q) and any(len(r) for r in q)
    db, q = cases["empty_database_source"]
    assert any(len(r) == 0 for r in db)
    db, q = cases["query_equals_database_source"]
    sk = Q.concat(db, q)
    want = Q.expected(sk, len(db), Q.CROSS)
    assert (0, len(db), len(db[0])) in [tuple(r) for r in want.tolist()]       # shared = the run's length
    db, q = cases["one_hash_sources"]
    assert all(len(r) == 1 for r in db + q)
    db, q = cases["keys_0_and_top"]
    assert any(0 in r and Q.TOP in r for r in db) and any(0 in r and Q.TOP in r for r in q)
    db, q = cases["one_key_held_by_all"]
    assert all(42 in r for r in db + q) and len(Q.expected(Q.concat(db, q), len(db), Q.CROSS)) == len(db) * len(q)
    db, q = cases["keys_outside_the_table"]
    tk = _table_keys(q)
    flat = [k for r in db for k in r]
    assert min(flat) < int(tk.min()) and max(flat) > int(tk.max())
    db, q = cases["identical_queries"]
    assert list(q[0]) == list(q[1])
    self_rows = Q.expected(Q.concat(db, q), len(db), Q.CROSS_AND_SELF)
    assert (len(db), len(db) + 1, len(q[0])) in [tuple(r) for r in self_rows.tolist()]


def test_mode_filter_partitions_the_full_table():
    db, q = Q.tile_case(65)
    sk = Q.concat(db, q)
    full = oracle.brute_pairs(sk.keys, sk.offsets)
    cross, both = Q.filter_mode(full, len(db), Q.CROSS), Q.filter_mode(full, len(db), Q.CROSS_AND_SELF)
    old = full[full["source_2"] < len(db)]
    assert len(old) + len(both) == len(full) and len(cross) < len(both)        # database x database + mode 1 = the union's table
    assert (cross["source_1"] < len(db)).all() and (cross["source_2"] >= len(db)).all()
    assert (both["source_1"] < both["source_2"]).all() and (both["shared"] > 0).all()
    dbk, dbo, qk, qo = Q.split(sk, len(db))
    assert dbo[0] == 0 and qo[0] == 0 and dbo[-1] == dbk.size and qo[-1] == qk.size and dbk.size + qk.size == sk.keys.size


def test_tile_cases_straddle_the_tile():
    for n_q in (63, 64, 65, 129):
        db, q = Q.tile_case(n_q)
        assert len(q) == n_q and len(db) == 40
        want = Q.expected(Q.concat(db, q), len(db), Q.CROSS)
        tiles = np.unique((want["source_2"] - len(db)) // 64)
        assert tiles.size == (n_q + 63) // 64                                  # every tile has rows
        assert len(want) < len(db) * n_q                                       # and some pairs share nothing


def test_long_run_case_lengths():
    db, q = Q.long_run_case()
    assert tuple(len(np.unique(r)) for r in db) == Q.LONG_RUN_LENGTHS
    assert {255, 256, 257, 1000} <= set(Q.LONG_RUN_LENGTHS) and min(Q.LONG_RUN_LENGTHS) < 255


def test_block_case_lengths_sit_on_both_sides_of_the_probe_blocks():
    db, q = Q.block_case()
    assert tuple(len(np.unique(r)) for r in db) == Q.BLOCK_RUN_LENGTHS
    for block in (256, 1024):                                                  # 64 lanes and 256 threads x 4 keys per step
        assert {block - 1, block, block + 1} <= set(Q.BLOCK_RUN_LENGTHS)
    assert min(Q.BLOCK_RUN_LENGTHS) < 64 and len(q) == 6 and all(len(np.unique(r)) == Q.BLOCK_QUERY_LENGTH for r in q)
    sk = Q.concat(db, q)
    cross, both = Q.expected(sk, len(db), Q.CROSS), Q.expected(sk, len(db), Q.CROSS_AND_SELF)
    assert set(cross["source_1"].tolist()) == set(range(len(db)))              # every run has a row
    assert len(both) == len(cross) + len(q) * (len(q) - 1) // 2                # and every pair of queries shares a key


@pytest.mark.parametrize("n_share", [31, 32, 33, 200])
def test_list_case_overflows_exactly_above_the_capacity(n_share):
    db, q = Q.list_case(n_share)
    sk = Q.concat(db, q)
    want = Q.expected(sk, len(db), Q.CROSS)
    assert (want["source_1"] == 0).sum() == n_share and (want["source_1"] == 1).sum() == 0
    assert all(len(r) == 2 for r in q)
    assert Q.expected_overflows(want, len(db), engine.QUERY_TILE_MAX, 32) == (1 if n_share > 32 else 0)
    # in mode 1 query i also touches the n_share - 1 - i queries above it
    both = Q.expected(sk, len(db), Q.CROSS_AND_SELF)
    assert Q.expected_overflows(both, len(db), engine.QUERY_TILE_MAX, 32) == (1 if n_share > 32 else 0) + max(0, n_share - 1 - 32)


def test_query_stats_layout_and_symbols():
    assert ctypes.sizeof(engine.QueryStats) == 120   # (= sizeof(ksp_query_stats), include/kspider_amd.h)
    for name in ("ksp_query_device", "ksp_query_host", "ksp_query_directory", "kspider_query", "kspider_pack", "ksp_pack_info", "ksp_pack_load"):
        assert name in engine.ABI_SYMBOLS and hasattr(engine.lib(), name)


def test_argument_refusals_need_no_device():
    """KSP_E_ARG comes before the device is chosen or anything is allocated."""
    sk = Q.concat([[1, 2]], [[2, 3]])
    dbk, dbo, qk, qo = Q.split(sk, 1)
    for args in [(None, dbo, qk, qo), (dbk, None, qk, qo), (dbk, dbo, None, qo), (dbk, dbo, qk, None),
                 (dbk, np.zeros(1, np.uint64), qk, qo), (dbk, dbo, qk, np.zeros(1, np.uint64)),
                 (dbk, np.array([1, 2], np.uint64), qk, qo), (dbk, dbo, qk, np.array([0, 2, 1], np.uint64))]:
        with pytest.raises(engine.KspError) as ei:
            engine.query_host(*args)
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.query_host(dbk, dbo, qk, qo, mode=2)
    assert ei.value.code == engine.KSP_E_ARG

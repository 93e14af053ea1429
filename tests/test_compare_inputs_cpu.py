"""The restatement of compare against rows worked out by hand, every input of the GPU tests against the property it is named for,
ksp_compare_values (host only) against the restatement and, within bounds derived from its operations, against values_exact (fractions
and 70-digit decimals), and the refusals that happen before a device is chosen.  No GPU."""
import ctypes
import json
import math
import os
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import compare_inputs as C
import compare_restate as R
from kspider_amd import engine


def test_the_restatement_gives_the_hand_computed_rows():
    db, q = C.hand_case()
    assert R.rows(db, q, R.CROSS_AND_SELF) == C.HAND_ROWS
    assert R.rows(db, q, R.CROSS) == [r for r in C.HAND_ROWS if r[0] == 0]
    assert R.rows([], db + q, R.CROSS_AND_SELF) == C.HAND_ROWS                  # all pairs of the union: the same numbering
    assert R.totals(db + q) == C.HAND_SUMS
    assert not [r for r in C.HAND_ROWS if 4 in r[:2]]                            # the disjoint sample has no row
    cosine, angular, w1, w2 = R.values(C.HAND_ROWS[3], 8, 26, 8, 26)             # identical samples
    assert (cosine, angular, w1, w2) == (1.0, 1.0, 1.0, 1.0)
    cosine, angular, w1, w2 = R.values(C.HAND_ROWS[0], 14, 78, 8, 26)
    assert cosine == 11 / (math.sqrt(78) * math.sqrt(26)) and abs(angular - (1 - 2 * math.acos(cosine) / math.pi)) < 1e-15 and (w1, w2) == (7 / 14, 4 / 8)
    assert 0 < angular < cosine < 1


def test_flat_rows_are_counts():
    db, q = C.random_case()
    for r in R.rows(C.flat(db), C.flat(q), R.CROSS_AND_SELF):
        assert r[2] == r[3] == r[4] == r[5] > 0


def test_random_case_shares_much_and_is_heavy_tailed():
    db, q = C.random_case()
    assert len(db) + len(q) == 40 and max(len(s) for s in db + q) <= 300 and min(len(s) for s in db + q) >= 1
    rows = R.rows(db, q, R.CROSS_AND_SELF)
    assert len(rows) > 0.8 * (40 * 39 // 2 - 12 * 11 // 2)                       # most pairs of the mode share a hash
    abunds = sorted(a for s in db + q for a in s.values())
    assert abunds[0] == 1 and abunds[len(abunds) // 2] <= 2 and abunds[-1] > 1000
    keys, abund, off = C.arrays(db)
    assert off[-1] == keys.size == abund.size and all((np.diff(keys[int(a):int(b)].astype(object)) > 0).all() for a, b in zip(off[:-1], off[1:]))


def test_width_case_crosses_the_words():
    db, q = C.width_case()
    rows = R.rows(db, q, R.CROSS_AND_SELF)
    assert rows == [(0, 1, 1, 2**64 - 2**33 + 1, C.TOP32, C.TOP32), (2, 3, 40, 120 * 2**30, 40 * 3 * 2**15, 40 * 2**15)]
    assert rows[0][3] > 2**63 and float(rows[0][3]) != rows[0][3]                # no signed and no double path holds it
    partial = [3 * 2**30 * i for i in range(1, 41)]
    assert partial[0] < 2**32 < partial[1] < 2**33 < partial[2] and partial[-1] == rows[1][3]
    assert max(R.totals(q)[1]) < 2**64


def test_limit_case_at_its_exact_value():
    assert sum(a * a for a in C.LIMIT_ABUNDS) == 2**64 - 1
    big, small = C.limit_case(2)
    assert R.totals([big])[1] == [2**64 - 1]
    big, small = C.limit_case(3)
    assert R.totals([big])[1] == [2**64 + 4] and R.rows([], [big, small], R.CROSS_AND_SELF) == [(0, 1, 1, C.TOP32, C.TOP32, 1)]


def test_seams_case_has_probes_in_front_of_inside_and_behind_tiles():
    _, q = C.seams_case()
    assert len(q) == 1100 and max(len(s) for s in q) <= 8 and len(q) > 2 * engine.COMPARE_TILE_MAX
    rows = R.rows([], q, R.CROSS_AND_SELF)
    tiles = {(r[0] // 512, r[1] // 512) for r in rows}
    assert tiles == {(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)}             # a probing query with holders in its own tile and in the tiles behind
    assert {r[1] - r[0] for r in rows} >= {1, 2, 3}                              # neighbours: across the seams of tiles of 1 and 3
    assert len(rows) > 1100


def test_list_case_overflows_the_forced_lists():
    _, q = C.list_case()
    rows = R.rows([], q, R.CROSS_AND_SELF)
    assert len(q) <= engine.COMPARE_TILE_MAX and len(rows) == 300 * 299 // 2
    touched = [sum(1 for r in rows if r[0] == s) for s in range(300)]            # the tile queries a probing source touches
    assert touched[0] == 299 and sum(t > 4 for t in touched) == 295 and sum(t > 1 for t in touched) == 298
    assert all(r[3] == (r[0] + 1) * (r[1] + 1) for r in rows)


def test_compare_values_equals_the_restatement():
    db, q = C.random_case()
    total, sq = R.totals(db + q)
    sizes = [len(s) for s in db + q]
    worst = 0.0
    for r in R.rows(db, q, R.CROSS_AND_SELF):
        got = engine.compare_values(r, sizes[r[0]], total[r[0]], sq[r[0]], sizes[r[1]], total[r[1]], sq[r[1]])
        want = R.values(r, total[r[0]], sq[r[0]], total[r[1]], sq[r[1]])
        worst = max(worst, max(abs(g - w) for g, w in zip(got, want)))
        assert all(0.0 <= g <= 1.0 for g in got)
    assert worst < 1e-12
    # identical samples: exactly 1, also where the roots do not multiply back (Σ a² = 2^64 - 1) and at the widest dot
    big = 2**64 - 1
    assert engine.compare_values((0, 1, 5, big, 10, 10), 5, 10, big, 5, 10, big)[:2] == (1.0, 1.0)
    _, wq = C.width_case()
    (r0, _), (_, wsq) = R.rows([], wq, R.CROSS_AND_SELF), R.totals(wq)
    got, want = engine.compare_values(r0, 1, C.TOP32, wsq[0], 2, C.TOP32 + 1, wsq[1]), R.values(r0, C.TOP32, wsq[0], C.TOP32 + 1, wsq[1])
    assert max(abs(g - w) for g, w in zip(got, want)) < 1e-12 and got[0] <= 1.0
    with pytest.raises(engine.KspError) as ei:
        engine.compare_values((0, 1, 1, 1, 1, 1), 1, 0, 0, 1, 1, 1)
    assert ei.value.code == engine.KSP_E_ARG
    assert engine.lib().ksp_compare_values(None, 1, 1, 1, 1, 1, 1, (ctypes.c_double * 4)()) == engine.KSP_E_ARG


def test_abi_mirror():
    assert engine.WEDGE_DTYPE.itemsize == ctypes.sizeof(engine.Wedge) == 40 and ctypes.sizeof(engine.CompareStats) == 128
    for name in ("ksp_compare_device", "ksp_compare_host", "ksp_compare_values", "kspider_compare"):
        assert name in engine.ABI_SYMBOLS and hasattr(engine.lib(), name)


def test_refusals_before_a_device_is_chosen(tmp_path):
    """NULL arguments, bad offsets, an unknown mode, n_db = 0 with CROSS, n_q = 0: KSP_E_ARG from the arguments alone — the device
    is -1, which a call that got as far as choosing one would refuse with KSP_E_HIP."""
    db, q = C.hand_case()
    dk, da, do = C.arrays(db)
    qk, qa, qo = C.arrays(q)
    none = np.zeros(1, np.uint64)
    cases = [(dk, da, do, None, qa, qo, 1), (dk, da, do, qk, qa, None, 1), (None, da, do, qk, qa, qo, 1), (dk, da, None, qk, qa, qo, 0),
             (dk, da, do + 1, qk, qa, qo, 1), (dk, da, do, qk, qa, qo[::-1].copy(), 1), (dk, da, do, qk, qa, qo, 2), (dk, da, do, qk, qa, qo, -1),
             (None, None, None, qk, qa, qo, 0), (dk, da, do, qk, qa, none, 1)]
    for *args, mode in cases:
        with pytest.raises(engine.KspError) as ei:
            engine.compare_host(*args, mode=mode, device=-1)
        assert ei.value.code == engine.KSP_E_ARG, (args, mode)
        with pytest.raises(engine.KspError) as ei:
            engine.compare_device(*(a if a is None or i in (2, 5) else a.ctypes.data for i, a in enumerate(args)), None, 0, mode=mode, device=-1)
        assert ei.value.code == engine.KSP_E_ARG, (args, mode)
    L = engine.lib()
    out, n = ctypes.c_void_p(), ctypes.c_uint64(0)
    assert L.ksp_compare_host(None, None, None, 0, qk.ctypes.data, None, qo.ctypes.data, len(q), 1, -1, None, ctypes.byref(n), None, None, None) == engine.KSP_E_ARG
    assert L.ksp_compare_host(None, None, None, 0, qk.ctypes.data, None, qo.ctypes.data, len(q), 1, -1, ctypes.byref(out), None, None, None, None) == engine.KSP_E_ARG
    assert L.ksp_compare_device(-1, None, None, None, 0, qk.ctypes.data, None, qo.ctypes.data, len(q), 1, None, 8, ctypes.byref(n), None, None, None) == engine.KSP_E_ARG
    # the file driver: refused from the arguments, and nothing is written
    prefix = str(tmp_path / "OUT")
    for args in [(None, 21, prefix), (str(tmp_path), 21, None), (str(tmp_path), -1, prefix)]:
        with pytest.raises(engine.KspError) as ei:
            engine.compare(*args)
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.compare(str(tmp_path), 21, prefix, against=str(tmp_path), matrix=True)
    assert ei.value.code == engine.KSP_E_ARG and "matrix" in str(ei.value)
    assert engine.lib().kspider_compare(str(tmp_path).encode(), None, 21, prefix.encode(), 1, 2) == engine.KSP_E_ARG
    assert list(tmp_path.iterdir()) == []


def test_the_file_driver_under_the_sanitizers(tmp_path):
    """The stand-alone sanitizer program (make asan-pack) runs kspider_compare up to the device call — a counted, a flat and a
    twice-listing signature are loaded and the flat one's abundances filled with ones, then the stub's engine refuses — and
    ksp_compare_values at the top of its range: no report, no file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "kspider_amd", "csrc"), "asan-pack"], stdout=subprocess.DEVNULL)
    sigs = tmp_path / "sigs"
    sigs.mkdir()
    for name, sig in {"counted": {"mins": [5, 3, 9], "abundances": [2, 7, 1]}, "flat": {"mins": [3, 4]}, "twice": {"mins": [9, 9, 1], "abundances": [1, 2, 3]}}.items():
        (sigs / (name + ".sig")).write_text(json.dumps([{"signatures": [dict(sig, ksize=21)]}]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(root, "kspider_amd", "lib", "pack_asan_check")
    for args in [(str(sigs), "21", str(tmp_path / "OUT")), (str(sigs), "21", str(tmp_path / "OUT"), str(sigs))]:
        p = subprocess.run([exe, "compare", *args], capture_output=True, text=True, env=env, timeout=120)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr and p.returncode == 0, p.stderr[-3000:]
        lines = p.stdout.splitlines()
        assert lines[0].split()[:2] == ["rc", str(engine.KSP_E_HIP)]
        assert lines[1].split() == ["values", "0", "1", "1", "1", "0.90000000000000002"]
    assert sorted(os.listdir(tmp_path)) == ["sigs"]


# ---- the inputs of tests/test_compare_edges_gpu.py ----------------------------------------------------------------------------
def test_block_case_sits_at_the_probe_s_trips():
    db, q = C.block_case()
    assert tuple(len(s) for s in db) == (255, 256, 257, 1023, 1024, 1025, 3) == C.BLOCK_RUN_LENGTHS
    assert len(q) == 12 and all(len(s) == C.BLOCK_QUERY_LENGTH == 600 for s in q)
    assert 600 > 2 * 256 and sum(n >= 1000 for n in C.BLOCK_RUN_LENGTHS) == 3    # a probing query: two full trips of a wave and a tail
    held = set().union(*q)
    for s in db:                                                                 # an entry lost at either end of a run changes a row
        run = sorted(s)
        assert set(run[:4]) & held and set(run[-4:]) & held and run[0] in held and run[-1] in held
        short = dict(s)
        del short[run[-1]]
        assert R.rows([short], q, R.CROSS) != R.rows([s], q, R.CROSS)
    abunds = sorted(a for s in db + q for a in s.values())
    assert abunds[0] == 1 and abunds[len(abunds) // 2] <= 2 and abunds[-1] > 1000
    assert {r[0] for r in R.rows(db, q, R.CROSS)} == set(range(7)) and len(R.rows(db, q, R.CROSS)) > 6 * 12


def test_lane_carry_case_carries_in_one_lane_only():
    lanes = 256                                                                  # the totals kernel: lane t reads entries t, t + 256, ...
    for accepted in (False, True):
        big, small = C.lane_carry_case(accepted)
        run = [big[h] for h in sorted(big)]
        assert len(run) == C.LANE_RUN == 300 > lanes and C.LANE_AT + lanes < len(run) and set(small) & set(big)
        order = sorted(range(len(run)), key=lambda j: -run[j])
        assert sorted(order[:2]) == [C.LANE_AT, C.LANE_AT + lanes]              # the two largest: one lane's entries
        lane_sq = [sum(a * a for a in run[t::lanes]) for t in range(lanes)]
        others = sum(lane_sq) - lane_sq[C.LANE_AT]
        if accepted:
            assert sum(lane_sq) == 2**64 - 1 == R.totals([big])[1][0] and max(lane_sq) < 2**64          # no lane wraps, nor the sum
            assert run[C.LANE_AT] == C.LIMIT_ABUNDS[0] and run[C.LANE_AT + lanes] == C.LIMIT_ABUNDS[1] and run[0] == C.LIMIT_ABUNDS[2]
            assert sum(a * a for j, a in enumerate(run) if j not in (0, C.LANE_AT, C.LANE_AT + lanes)) == 19 * 19 + 2 * 2
        else:
            assert run[C.LANE_AT] == run[C.LANE_AT + lanes] == C.TOP32 and sorted(run)[:-2] == [1] * 298
            assert sum(lane_sq) == 2**65 - 2**34 + 300 >= 2**64
            # the lane's own sum wraps once; what is left of it and all the other lanes' sums stay far below 2^64 in any order, so
            # no add to the workgroup's sum wraps: the lane-local carry is the only one
            assert 2**64 <= lane_sq[C.LANE_AT] < 2**65 and others == 298
            assert (lane_sq[C.LANE_AT] - 2**64) + others < 2**64 - 2**33
    db, q = C.lane_carry_many()
    over = [sq >= 2**64 for sq in R.totals(db + q)[1]]
    assert over == [False, True, False, True, True, False, True, False]          # the smallest: database source 1; of the queries: 0


def test_mass_width_case_crosses_the_word_in_every_sum():
    first, second = C.mass_width_case()
    shared = sorted(set(first) & set(second))
    assert len(shared) == C.MASS_N >= 2048 and len(first) > len(shared) < len(second)
    (row,) = R.rows([first], [second], R.CROSS)
    assert row == R.rows([], [first, second], R.CROSS_AND_SELF)[0] and row[2] == C.MASS_N
    assert min(row[3:]) >= 2**32 and max(R.totals([first, second])[1]) < 2**64 and min(R.totals([first, second])[0]) >= 2**32
    assert len({first[h] for h in shared}) > 1 and len({second[h] for h in shared}) > 1
    assert all(abs(first[h] - 2**21) < 8 and abs(second[h] - 2**20) < 8 for h in shared)
    for terms in ([first[h] * second[h] for h in shared], [first[h] for h in shared], [second[h] for h in shared]):
        crossings, total = 0, 0
        for v in terms:                                                          # the low word carries again and again, in entry order
            crossings += (total + v) >> 32 != total >> 32
            total += v
        assert crossings >= 4 and max(terms) < 2**63


def test_check_seams_variants_are_the_faults_they_are_named_for():
    db, q = C.check_seams_base()
    base = (C.arrays(db), C.arrays(q))
    assert R.refusal(*base) is None and all(len(s) == C.SEAM_RUN == 300 for s in db + q)
    firsts, lasts = [min(s) for s in db + q], [max(s) for s in db + q]
    assert lasts[0] == firsts[1] and all(lasts[i] > firsts[i + 1] for i in range(1, 7))     # legal: a run ascends inside its source only
    assert len(R.rows(db, q, R.CROSS_AND_SELF)) > 4
    variants = C.check_seams_variants()
    assert len(variants) == 8
    changed = {}
    for name, (db_side, q_side, message) in variants.items():
        assert R.refusal(db_side, q_side) == message, name
        changed[name] = [(side, kind, int(i)) for side, got, was in (("database", db_side, base[0]), ("query", q_side, base[1]))
                         for kind, a, b in (("key", got[0], was[0]), ("abund", got[1], was[1])) for i in np.nonzero(a != b)[0]]
        assert (db_side[2] == base[0][2]).all() and (q_side[2] == base[1][2]).all()
    assert changed["equal_at_255_256"] == [("query", "key", 300 + 256)] and changed["descending_at_255_256"] == [("database", "key", 300 + 256)]
    assert changed["zero_at_256"] == [("query", "abund", 600 + 256)] and changed["zero_at_the_last_entry"] == [("database", "abund", 1199)]
    qk = variants["equal_at_255_256"][1][0]
    assert qk[555] == qk[556] < qk[557] and qk[554] < qk[555]
    dk = variants["descending_at_255_256"][0][0]
    assert dk[554] < dk[556] < dk[555] < dk[557]
    # several faulty sources: the smallest in the common numbering is not the first in either side's array order of faults alone
    assert [c[:2] for c in changed["bad_runs_on_both_sides"]] == [("database", "key"), ("query", "key"), ("query", "key")]
    assert [c[:2] for c in changed["bad_runs_in_the_queries"]] == [("query", "key"), ("query", "key")]
    later = variants["order_fault_behind_a_zero"]
    assert (later[0][1] == 0).sum() == 1 and "query source 3" in later[2]       # the zero is in database source 0, the order fault behind it


def test_empties_case_has_empty_sources_where_it_says():
    db, q = C.empties_case()
    assert [bool(s) for s in db] == [False, True, False] and [bool(s) for s in q] == [True, True, False, False, True, False]
    for mode in (R.CROSS, R.CROSS_AND_SELF):
        rows = R.rows(db, q, mode)
        named = {r[0] for r in rows} | {r[1] for r in rows}
        assert named == ({1, 3, 4, 7} if rows else set()) and len(rows) == (3 if mode == R.CROSS else 6)
    total, sq = R.totals(db + q)
    assert [t == 0 for t in total] == [s == 0 for s in sq] == [not s for s in db + q]
    _, _, off = C.arrays(q)
    assert off[2] == off[3] == off[4] and off[5] == off[6] and [int(off[i + 2] - off[i]) > 0 for i in (0, 2, 4)] == [True, False, True]
    # sides without a single key pass the argument check: the refusal is the missing device's
    empty, full = C.arrays([{}, {}, {}]), C.arrays(q)
    for sides in ((empty, full), (C.arrays(db), C.arrays([{}] * 6)), (empty, C.arrays([{}] * 6))):
        with pytest.raises(engine.KspError) as ei:
            engine.compare_host(*sides[0], *sides[1], mode=R.CROSS, device=-1)
        assert ei.value.code == engine.KSP_E_HIP, str(ei.value)


def test_full_tile_case_fills_a_tile_and_one_more():
    _, q = C.full_tile_case()
    assert len(q) == C.FULL_TILE_QUERIES == engine.COMPARE_TILE_MAX + 1 and all(len(s) == 2 and s[77] == i + 1 for i, s in enumerate(q))
    rows = R.rows([], q, R.CROSS_AND_SELF)
    assert len(rows) == 513 * 512 // 2 == 131328 and all(r[2:] == (1, (r[0] + 1) * (r[1] + 1), r[0] + 1, r[1] + 1) for r in rows)
    assert (0, 511, 1, 512, 1, 512) in rows and (511, 512, 1, 512 * 513, 512, 513) in rows                # tag 511, and the tile of one
    assert C.expected_overflows(rows, 0, 512, engine.COMPARE_LIST_MAX) == sum(511 - s > 256 for s in range(512)) == 255
    assert C.expected_overflows(R.rows(*C.list_case(), R.CROSS_AND_SELF), 0, 512, 4) == 295                # test_touched_list's count


def test_extreme_keys_cases_hold_the_keys_they_say():
    cases = C.extreme_keys_cases()
    db, q = cases["ends"]
    for side in (db, q):
        assert any(s.get(0, 0) > 1 and s.get(C.TOP64, 0) > 1 and len(s) > 2 for s in side)
        assert any(0 in s and C.TOP64 not in s for s in side) and any(C.TOP64 in s and 0 not in s for s in side)
    keys, _, _ = C.arrays(q)
    assert int(keys.max()) == 2**64 - 1 and int(keys.min()) == 0
    rows = R.rows(db, q, R.CROSS_AND_SELF)
    assert any(r[2] == 3 for r in rows) and any(r[2] == 2 and r[3] == 5 * 6 + 7 * 6 for r in rows)         # d0 x q4: hashes 0 and 2^64 - 1
    db, q = cases["one_bucket"]
    table = sorted(set().union(*q))
    assert len(table) == 64 and len({k >> 57 for k in table}) == 1 and min(table) == 2**63                 # 64 keys: 4 directory bits of 64
    probes = set().union(*db)
    assert probes & set(table) and any(table[0] < k < table[-1] and k not in table for k in probes)
    assert any(k > table[-1] for k in probes) and any(k < table[0] for k in probes)
    assert set(db[3]) == set(table) and len(R.rows(db, q, R.CROSS)) == 1 + 2 + 8                          # misses, two hits, the largest, all
    db, q = cases["only_zero"]
    assert all(set(s) == {0} for s in q) and R.rows(db, q, R.CROSS_AND_SELF) == [(0, 3, 1, 15, 5, 3), (0, 4, 1, 20, 5, 4), (2, 3, 1, 27, 9, 3),
                                                                               (2, 4, 1, 36, 9, 4), (3, 4, 1, 12, 3, 4)]


# ---- ksp_compare_values against values_exact ----------------------------------------------------------------------------------
U = Decimal(2) ** -53                                                            # the unit roundoff of a double


def test_the_exact_acos_is_acos():
    for num, den_sq in [(1, 4), (3, 10), (11, 78 * 26), (999, 10**6), (1, 10**12), (10**6 - 1, 10**12), (2**64 - 2**33 + 1, (2**64 - 1)**2)]:
        angle = R.acos_exact(num, den_sq)
        c = R._ctx().divide(Decimal(num), Decimal(den_sq).sqrt(R._ctx()))
        assert abs(R.cos_exact(angle) - c) < Decimal(10) ** -55                  # cos(acos c) = c
        x = num / math.sqrt(den_sq)
        assert abs(float(angle) - math.acos(x)) <= 4 * 2.0**-53 * (1 + 1 / math.sqrt((1 - x) * (1 + x)))   # math.acos, as far as its argument allows
    assert abs(R.pi_exact() - Decimal("3.14159265358979323846264338327950288419716939937510582097494")) < Decimal(10) ** -58
    assert float(R.pi_exact()) == math.pi and R.values_exact((0, 1, 3, 26, 8, 8), 8, 26, 8, 26) == (1, 1, 1, 1)


def _within_the_derived_bounds(row, sum_1, sq_1, sum_2, sq_2):
    """ksp_compare_values against values_exact.  The cosine is the quotient of a converted integer by the product of two roots of
    converted integers: seven roundings, two of them halved by the root, each at most 2^-53 relative — within 8 · 2^-53 of the exact
    value.  A containment is the quotient of two converted integers.  acos turns an error δ of the cosine into δ / sqrt(1 - c²);
    its own rounding, the division by π, π's and the subtraction add less than 4 · 2^-53 to a value of at most 1."""
    got = [Decimal(g) for g in engine.compare_values(row, 1, sum_1, sq_1, 1, sum_2, sq_2)]
    cosine, angular, w1, w2 = R.values_exact(row, sum_1, sq_1, sum_2, sq_2)
    assert all(0 <= g <= 1 for g in got)
    if cosine == 1:
        assert got[0] == 1 and got[1] == 1
    else:
        delta = 8 * U * cosine
        assert abs(got[0] - cosine) <= delta, (row, got[0], cosine)
        root = (Decimal(sq_1 * sq_2 - row[3] * row[3]) / Decimal(sq_1 * sq_2)).sqrt(R._ctx())              # sqrt(1 - c²), from the integers
        assert abs(got[1] - angular) <= 2 / R.pi_exact() * delta / root + 4 * U, (row, got[1], angular)
    assert abs(got[2] - w1) <= 2 * U * w1 and abs(got[3] - w2) <= 2 * U * w2, (row, got[2:], w1, w2)
    return got


def test_compare_values_on_the_random_rows_within_the_derived_bounds():
    db, q = C.random_case()
    total, sq = R.totals(db + q)
    rows = R.rows(db, q, R.CROSS_AND_SELF)
    assert len(rows) > 500
    for r in rows:
        _within_the_derived_bounds(r, total[r[0]], sq[r[0]], total[r[1]], sq[r[1]])


def test_compare_values_on_the_widest_rows_within_the_derived_bounds():
    top = 2**64 - 1
    assert _within_the_derived_bounds((0, 1, 5, top, top, top), top, top, top, top)[:2] == [1, 1]          # parallel at the top: exactly 1
    _, wq = C.width_case()
    (r0, r1), (wsum, wsq) = R.rows([], wq, R.CROSS_AND_SELF), R.totals(wq)
    _within_the_derived_bounds(r0, wsum[0], wsq[0], wsum[1], wsq[1])
    _within_the_derived_bounds(r1, wsum[2], wsq[2], wsum[3], wsq[3])
    # totals at 2^64 - 1 with a dot and masses the conversion to double has to round: one above a power of two, one below the top
    for dot in (2**64 - 2**33 + 1, 2**63 + 1, 2**53 + 1, top - 1, 1):
        for mass in (top, top - 2**10, 2**63 + 2**10 + 1, 2**53 + 1, 1):
            _within_the_derived_bounds((0, 1, 1, dot, mass, mass), top, top, top, top)
            _within_the_derived_bounds((0, 1, 1, dot, min(mass, top - 2**11), min(mass, 2**63 + 3)), top - 2**11, top, 2**63 + 3, top)


def test_compare_values_on_nearly_parallel_and_nearly_orthogonal_pairs():
    seen = []
    for pairs in (C.nearly_parallel_pairs(), C.nearly_orthogonal_pairs()):
        for a, b in pairs:
            assert len(a) in (200, 201) and len(a) == len(b)
            (row,) = R.rows([a], [b], R.CROSS)
            total, sq = R.totals([a, b])
            got = _within_the_derived_bounds(row, total[0], sq[0], total[1], sq[1])
            seen.append((float(R.values_exact(row, total[0], sq[0], total[1], sq[1])[0]), float(got[0])))
    parallel, orthogonal = seen[:6], seen[6:]
    assert all(1 - 1e-3 < c < 1 for c, _ in parallel[:1]) and all(c > 1 - 1e-3 for c, _ in parallel) and max(g for _, g in parallel) > 1 - 8 * 2.0**-53   # within the cosine's own bound of 1
    assert all(0 < c < 1e-3 for c, _ in orthogonal) and min(c for c, _ in orthogonal) < 1e-15
    a, b = C.nearly_parallel_pairs()[0]
    assert sum(a[h] != b[h] for h in a) == 1 and sum(b.values()) - sum(a.values()) == 1

"""The restatement of compare against rows worked out by hand, every input of the GPU tests against the property it is named for,
ksp_compare_values (host only) against the restatement, and the refusals that happen before a device is chosen.  No GPU."""
import ctypes
import json
import math
import os
import subprocess

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

"""`kSpider pairwise --estimate-ani` without a GPU: kspider_estimate_ani against the Python restatement of
ks_pairwise.py:29-84 (tests/ani_restate.py) byte for byte, its loud failures, and the device's code path (exact 6-digit
decimal + table, run on the host through ksp_ani_values) against the text definition bit for bit."""
import os
import random
import shutil

import numpy as np
import pytest

from ani_restate import ani_of_floats, estimate_ani as restated, float_text
from kspider_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "clusters")


def _stage(tag, tmp_path, k):
    d = tmp_path / tag
    d.mkdir()
    for f in ("sigs_kSpider_pairwise.tsv", "sigs_kSpider_seqToKmersNo.tsv"):
        shutil.copy(os.path.join(GOLD, tag, f), d / f)
    (d / "sigs.extra").write_text(f"{k}\n")
    return str(d / "sigs")


def _ani_path(prefix):
    return prefix + "_kSpider_pairwise.ani_col.tsv"


@pytest.mark.parametrize("tag", ["setA", "setB"])
@pytest.mark.parametrize("k", [1, 2, 21, 31, 51])
def test_estimate_ani_equals_restatement_on_golden_tsvs(tag, k, tmp_path):
    prefix = _stage(tag, tmp_path, k)
    engine.estimate_ani(prefix, 3, 1000)
    got = open(_ani_path(prefix), "rb").read()
    assert got == restated(prefix, 1000)
    assert got.count(b"\n") == sum(1 for _ in open(prefix + "_kSpider_pairwise.tsv"))
    assert not os.path.exists(_ani_path(prefix) + ".partial")


TEXTS = ["0", "0.0001", "0.000100001", "0.999899", "0.9999", "1", "1e-05", "inf", "0.101562", "0.5", "0.0106383"]


def _hand_made(tmp_path, k=21, rows=None, kmers_ids=range(1, 41), extra=None):
    prefix = str(tmp_path / "hand")
    rng = random.Random(7)
    if rows is None:
        rows = []
        for i in range(1, 41):
            for j in range(i + 1, 41, 3):
                rows.append(f"{i}\t{j}\t{rng.randint(1, 9)}\t{rng.choice(TEXTS)}\t0.5\t{rng.choice(TEXTS)}")
        rng.shuffle(rows)
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write("source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n")
        f.write("".join(r + "\n" for r in rows))
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n")
        f.write("".join(f"{n}\t{i}\t{100 + i}\n" for n, i in enumerate(kmers_ids, 1)))
    if extra is not False:
        with open(prefix + ".extra", "w") as f:
            f.write(extra if extra is not None else f"{k}\n")
    return prefix


@pytest.mark.parametrize("k", [1, 21, 51])
def test_estimate_ani_hand_made_texts_any_row_order(tmp_path, k):
    prefix = _hand_made(tmp_path, k)
    engine.estimate_ani(prefix, 4, 10)
    got = open(_ani_path(prefix), "rb").read()
    assert got == restated(prefix, 10)
    vals = set(got.decode().split("\n")[1:-1])
    assert "0.0" in vals and "1.0" in vals   # the two constants are reached


@pytest.mark.parametrize("case", ["nan", "-nan", "unknown_id", "scale0", "no_extra", "bad_extra", "k0", "truncated"])
def test_estimate_ani_fails_loudly_and_leaves_no_file(tmp_path, case):
    rows = ["1\t2\t3\t0.5\t0.5\t0.75", "2\t3\t1\t0.25\t0.3\t0.4"]
    kw = {}
    scale = 1000
    if case in ("nan", "-nan"):
        rows.append(f"1\t3\t0\t{case}\t{case}\t{case}")
    elif case == "unknown_id":
        rows.append("1\t99\t1\t0.1\t0.1\t0.1")
    elif case == "scale0":
        scale = 0
    elif case == "no_extra":
        kw["extra"] = False
    elif case == "bad_extra":
        kw["extra"] = "twenty-one\n"
    elif case == "k0":
        kw["extra"] = "0\n"
    elif case == "truncated":
        rows.append("1\t3\t1\t0.1")
    prefix = _hand_made(tmp_path, rows=rows, kmers_ids=[1, 2, 3], **kw)
    with pytest.raises(engine.KspError):
        engine.estimate_ani(prefix, 2, scale)
    assert not os.path.exists(_ani_path(prefix))
    assert not os.path.exists(_ani_path(prefix) + ".partial")
    if case not in ("k0",):
        with pytest.raises(Exception):
            restated(prefix, scale)


def test_estimate_ani_needs_the_pairwise_tsv(tmp_path):
    prefix = _hand_made(tmp_path)
    os.remove(prefix + "_kSpider_pairwise.tsv")
    with pytest.raises(engine.KspError):
        engine.estimate_ani(prefix, 1, 1000)
    assert not os.path.exists(_ani_path(prefix))


def test_python_repr_of_the_column():
    vals = [0.0, 1.0, 0.0001, 5e-05, 5.00005e-05, 0.5, 0.123456789, 1e16, 1.5e-7, 0.99995, 123.0, 0.30078125,
            2.0 ** -20, 1 / 3, 0.1 + 0.2]
    rng = np.random.default_rng(3)
    vals += list(rng.random(2000)) + list(10.0 ** rng.uniform(-9, 3, 2000))
    for v in vals:
        assert engine.format_ani(v) == repr(float(v))


def _check_table_equals_text(mn, mx, k):
    rc0, text = engine.ani_values(mn, mx, k, via_table=False)
    rc1, table = engine.ani_values(mn, mx, k, via_table=True)
    assert rc0 == 0 and rc1 == 0
    bad = np.flatnonzero(text.view(np.uint64) != table.view(np.uint64))
    assert bad.size == 0, [(float(mn[i]), float(mx[i]), text[i], table[i]) for i in bad[:5]]
    return text


def _near(x, ulps):
    b = np.float32(x).view(np.uint32).astype(np.int64)
    return (b + np.arange(-ulps, ulps + 1)).astype(np.uint32).view(np.float32)


def _small_ratios():
    n = np.arange(1, 2049, dtype=np.int64)
    s = np.concatenate([np.arange(0, m + 1) for m in n])
    d = np.repeat(n, n + 1)
    return (s.astype(np.float32) / d.astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 2, 21, 31, 51])
def test_table_path_equals_text_definition(k):
    """The device's code path (exact 6-digit decimal, half to even, table lookup) against '%.6g' -> strtod -> pow."""
    r = _small_ratios()                                                       # every s/n, n <= 2048 (13/128: a tie)
    edges = np.concatenate([_near(0.0001, 64), _near(0.9999, 64), _near(1.0, 64), _near(9e-5, 64),
                            np.array([0.0, np.inf, 13 / 128, 0.1015625], dtype=np.float32)])
    rng = np.random.default_rng(k)
    rnd = rng.uniform(1e-5, 1.0, 10_000_000).astype(np.float32)              # 10^7 random floats in [1e-5, 1]
    for a in (r, edges, rnd):
        _check_table_equals_text(a, a[::-1].copy(), k)


@pytest.mark.parametrize("k", [1, 21])
def test_table_path_equals_restatement(k):
    r = _small_ratios()
    rng = np.random.default_rng(100 + k)
    pick = np.concatenate([r[rng.integers(0, r.size, 100_000)], _near(0.0001, 64), _near(0.9999, 64),
                           rng.uniform(1e-5, 1.0, 100_000).astype(np.float32)])
    mx = pick[rng.permutation(pick.size)]
    got = _check_table_equals_text(pick, mx, k)
    want = np.array([ani_of_floats(a, b, k) for a, b in zip(pick.tolist(), mx.tolist())])
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    assert float_text(13 / 128) == "0.101562"


def test_ani_value_single_and_nan():
    out = engine.ctypes.c_double()
    L = engine.lib()
    for via in (0, 1):
        assert L.ksp_ani_value(0.25, 0.5, 21, via, engine.ctypes.byref(out)) == 0
        assert out.value == ani_of_floats(0.25, 0.5, 21)
        assert L.ksp_ani_value(float("nan"), 0.5, 21, via, engine.ctypes.byref(out)) == 1
        assert L.ksp_ani_value(0.25, 0.5, 0, via, engine.ctypes.byref(out)) == 1

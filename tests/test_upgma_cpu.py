"""The average-linkage tree without a GPU: the restatement of tests/upgma_restate.py against scipy, its three forms against each other,
ksp_upgma_before against Python integers, the properties of the GPU tests' inputs (tests/upgma_inputs.py), and the host-only
kspider_cluster_from_upgma with its refusals on hand-written tables."""
import glob
import os

import numpy as np
import pytest

import upgma_inputs as ui
import upgma_restate as ur
from kspider_amd import engine


def _tuples(rows):
    return [tuple(int(x) for x in r) for r in rows.tolist()]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(20))
def test_restatement_against_scipy_average_linkage(seed):
    """Complete graphs of 12 nodes, values k / 65536: memberships of every merge equal scipy's, heights within 1e-12 (at most 11
    nested weighted means of values <= 1, a few roundings of 2^-53 each)."""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    n = 12
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    k = rng.integers(1, 65537, len(a))
    v = np.zeros((n, n))
    v[a, b] = v[b, a] = k / 65536.0
    rows = ur.sequential_small(n, a, b, (k.astype(np.uint64) << np.uint64(16)).tolist())
    sims = [ur.order_key(r)[0] for r in rows]
    assert len(rows) == n - 1 and len(set(sims)) == n - 1                  # pairwise distinct merge similarities: no tie for scipy to break
    Z = linkage(squareform(1.0 - v, checks=False), "average")
    members = {i: frozenset([i]) for i in range(n)}
    mine = {i: frozenset([i]) for i in range(n)}
    for i, (lo, hi, s, slo, shi) in enumerate(rows):
        x, y, height, count = Z[i]
        got = frozenset([members[int(x)], members[int(y)]])
        assert got == frozenset([mine[lo], mine[hi]]), (seed, i)
        members[n + i] = members[int(x)] | members[int(y)]
        mine[lo] = mine[lo] | mine.pop(hi)
        assert len(members[n + i]) == count == slo + shi
        assert abs(height - (1.0 - s / (slo * shi) / ur.TWO32)) <= 1e-12, (seed, i)


def test_the_three_forms_agree_on_500_tie_heavy_multigraphs():
    longest = 0
    for seed in range(500):
        n, a, b, q = ui.tie_heavy_small(seed)
        want = ur.sequential_small(n, a, b, q.tolist())
        rows, rounds, run = ur.parallel_small(n, a, b, q.tolist())
        assert rows == want, seed                                         # the theorem of DESIGN.md 7m
        assert rounds <= max(0, n - 1) and run <= 4, (seed, rounds, run)  # progress, short runs
        longest = max(longest, run)
        assert _tuples(ur.merges(n, a, b, q)) == want, seed
        keys = [ur.order_key(r) for r in want]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)        # strictly descending in the order
    assert longest == 4


def test_paths_need_many_rounds_and_agree():
    for equal in (False, True):
        n, a, b, v = ui.path(40, equal)
        q = ur.q_of(v)
        rows, rounds, _ = ur.parallel_small(n, a, b, q.tolist())
        assert rows == ur.sequential_small(n, a, b, q.tolist()) == _tuples(ur.merges(n, a, b, q)) and len(rows) == n - 1
        assert rounds > (20 if not equal else 3), (equal, rounds)


def test_q_of():
    v = np.array([0.0, 1.0, 0.5, 2.0 ** -32, 2.0 ** -33, np.nan, 1.0000001, np.inf, -0.5, 1 / 3], dtype=np.float32)
    assert ur.q_of(v).tolist() == [0, 1 << 32, 1 << 31, 1, 0, 0, 0, 0, 0, int(float(np.float32(1 / 3)) * 2 ** 32)]


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------

def test_input_properties():
    assert ui.CHUNK == engine.UPGMA_CHUNK_EDGES and ur.ROW_DTYPE == engine.UPGMA_ROW_DTYPE and ur.ROW_DTYPE.itemsize == 24
    n, a, b, v = ui.two_pairs_all_cross()
    rows, rounds, run = ur.parallel_small(n, a, b, ur.q_of(v).tolist())
    assert run == 4 and rounds == 2 and [r[:2] for r in rows] == [(0, 1), (2, 3), (0, 2)]
    for equal in (False, True):
        n, a, b, v = ui.path(300, equal)
        rows, rounds, _ = ur.parallel_small(n, a, b, ur.q_of(v).tolist())
        assert len(rows) == 299 and (rounds > 150 or equal), rounds
    (n, a, b, v), part = ui.ignored_records()
    assert len(ur.pairs_of(n, a, b, ur.q_of(v).tolist())) == 1 and part == 5000
    n, a, b, v = ui.hub(equal=False)
    assert len(set(v.tolist())) == 5000 and v.min() > 0 and v.max() < 1


def test_the_hostile_input_is_hostile():
    """The rows with every cross product truncated to 64 bits differ from the true ones, and the deciding comparison is the one the
    docstring of the input names: its true cross products differ only above bit 64."""
    n, a, b, v = ui.hostile_cross_product()
    q = ur.q_of(v)
    want, wrong = ur.merges(n, a, b, q), ur.merges(n, a, b, q, trunc=True)
    assert len(want) == len(wrong) == 4000 and (want != wrong).any()
    assert tuple(want[0])[:2] == (4000, 4001) and tuple(want[-1]) == (0, 2000, 1999 << 20, 2000, 2000)
    x = int(want[0]["sum_q"]) * 4000000
    y = int(want[-1]["sum_q"])
    assert x >> 64 == 1 and (x & (2 ** 64 - 1)) < y < 2 ** 64 < x
    pair1, pair2 = (int(want[0]["sum_q"]), 1, 1, 4000, 4001), (y, 2000, 2000, 0, 2000)
    assert ur.before(pair1, pair2) and not ur.before(pair1, pair2, bits=64)
    assert engine.upgma_before(pair1, pair2) and not engine.upgma_before(pair2, pair1)


# ---- ksp_upgma_before ----------------------------------------------------------------------------------------------------------

def test_upgma_before_against_python_integers():
    big = 2 ** 32 - 1
    pairs = [(5, 1, 1, 0, 1), (5, 1, 1, 0, 2), (5, 1, 1, 1, 2), (10, 2, 1, 0, 1), (10, 1, 2, 3, 4), (5, 1, 1, 0, 1),
             (2 ** 64 - 1, big, big, 7, 9), (2 ** 64 - 2, big, big, 7, 9), (2 ** 64 - 1, big, big - 1, 7, 9), (2 ** 64 - 1, big, big, 6, 9),
             (2 ** 63, big, big, 1, 2), (2 ** 63 + 1, big, big, 1, 2), (2 ** 32, 2 ** 16, 2 ** 16, 4, 5), (2 ** 32 + 1, 2 ** 16, 2 ** 16, 4, 5),
             (2 ** 32 - 1, 2 ** 16, 2 ** 16, 4, 5), (2 ** 33, 2 ** 16, 2 ** 17, 4, 6), (1, big, big, 0, 1), (1, 1, 1, 0, 1), (2 ** 64 - 1, 1, 1, 0, 1),
             (2 ** 63, 2 ** 31, 2 ** 31 + 1, 2, 3), (2 ** 63 + 2 ** 31, 2 ** 31 + 1, 2 ** 31, 2, 4)]
    seen = set()
    for p1 in pairs:
        for p2 in pairs:
            x, y = p1[0] * p2[1] * p2[2], p2[0] * p1[1] * p1[2]
            seen.add((max(x, y) >= 2 ** 64, max(x, y) >= 2 ** 127, x == y))
            assert engine.upgma_before(p1, p2) == ur.before(p1, p2), (p1, p2)
    assert {(False, False, False), (True, False, False), (True, True, False), (True, False, True), (False, False, True)} <= seen
    assert not engine.upgma_before(pairs[0], pairs[0])                     # equal everything: neither is before
    for bad in ((1, 0, 1, 0, 1), (1, 1, 0, 0, 1)):
        with pytest.raises(engine.KspError) as ei:
            engine.upgma_before(bad, pairs[0])
        assert ei.value.code == engine.KSP_E_ARG
    assert engine.lib().ksp_upgma_before(1, 1, 1, 0, 1, 1, 1, 1, 0, 2, None) == engine.KSP_E_ARG


# ---- kspider_cluster_from_upgma: host only ------------------------------------------------------------------------------------

NAMES = ["a", "b", "c", "d", "e"]
TABLE = ur.rows_of([(0, 1, 1 << 32, 1, 1), (2, 3, 3 << 30, 1, 1), (0, 2, 5 << 30, 2, 2)])   # averages 1, 0.75, 0.3125


def _write(prefix, table_text):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(NAMES)}\n" + "".join(f"{i + 1} {n}\n" for i, n in enumerate(NAMES)))
    with open(prefix + "_kSpider_upgma_max_cont.tsv", "w") as f:
        f.write(table_text)


@pytest.mark.parametrize("cutoff, want", [(0.0, "a,b,c,d\ne\n"), (1.0, "a,b\nc\nd\ne\n"), (0.75, "a,b\nc,d\ne\n"), (0.3125, "a,b,c,d\ne\n"),
                                          (0.31250001, "a,b\nc,d\ne\n")])
def test_cluster_from_upgma_on_a_hand_written_table(tmp_path, cutoff, want):
    prefix = str(tmp_path / "ix")
    _write(prefix, ur.table_text("max_cont", TABLE))
    engine.cluster_from_upgma(prefix, "max_cont", cutoff)
    path = prefix + "_kSpider_clusters_upgma_max_cont_" + repr(cutoff * 100) + "%.tsv"
    with open(path) as f:
        assert f.read() == want == ur.cluster_text(NAMES, ur.cut_labels(5, TABLE, cutoff))
    assert not glob.glob(str(tmp_path / "*.partial"))


def test_cluster_from_upgma_refusals(tmp_path):
    prefix = str(tmp_path / "ix")
    good = ur.table_text("max_cont", TABLE)
    _write(prefix, good)
    before = sorted(os.listdir(tmp_path))
    for dist, cutoff, code in (("max_cont", -0.1, engine.KSP_E_ARG), ("max_cont", 1.5, engine.KSP_E_ARG), ("max_cont", float("nan"), engine.KSP_E_ARG),
                               ("ani", 0.5, engine.KSP_E_ARG), ("jaccard", 0.5, engine.KSP_E_ARG), ("min_cont", 0.5, engine.KSP_E_IO)):
        with pytest.raises(engine.KspError) as ei:
            engine.cluster_from_upgma(prefix, dist, cutoff)
        assert ei.value.code == code, (dist, cutoff)
    lines = good.split("\n")
    for bad in ("\n".join(lines[:2] + ["1\t2"] + lines[2:]), good.replace("\t3221225472\t", "\tmany\t"), good.replace("1\t2\t1\t", "1\t9\t1\t"),
                good.replace("\t2\t2\t4\n", "\t0\t2\t2\n"), good.replace("\t4294967296\t", "\t-4294967296\t")):
        assert bad != good
        _write(prefix, bad)
        with pytest.raises(engine.KspError) as ei:
            engine.cluster_from_upgma(prefix, "max_cont", 0.5)
        assert ei.value.code == engine.KSP_E_IO
    assert sorted(os.listdir(tmp_path)) == before


def test_file_writers_restated_by_hand():
    assert ur.table_text("max_cont", TABLE) == ("source_1\tsource_2\tmax_cont_average\tsum_q\tsize_1\tsize_2\tmerged_size\n"
                                                "1\t2\t1\t4294967296\t1\t1\t2\n3\t4\t0.75\t3221225472\t1\t1\t2\n1\t3\t0.3125\t5368709120\t2\t2\t4\n")
    assert ur.newick_text(NAMES, TABLE) == "(((a:0,b:0):0.6875,(c:0.25,d:0.25):0.4375):0.3125,e:1);\n"
    assert ur.newick_text(["x"], TABLE[:0]) == "x;\n" and ur.newick_text(NAMES[:2], TABLE[:1]) == "(a:0,b:0);\n"
    assert (ur.read_table(ur.table_text("max_cont", TABLE), "max_cont") == TABLE).all()

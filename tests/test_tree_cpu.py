"""The single-linkage tree without a GPU: kspider_cluster_from_tree — host only — over tree files written by
the restatement (tests/tree_restate.py) must give, byte for byte, the cluster file of oracle.ref_cluster over the FULL pairwise
TSV, at cut-offs that are printed values of rows and at the floats next to them; NaN and inf rows; refusals; the restatement
itself against scipy's single linkage; and the refusals of the device entries that are decided before any device call."""
import ctypes
import glob
import os
import re
import shutil

import numpy as np
import pytest

import tree_restate as tr
from kspider_amd import engine
from oracle import ref_cluster

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "clusters")
DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _rows(prefix, col):
    return [(int(p[0]), int(p[1]), p[col]) for p in (l.rstrip("\n").split("\t") for l in list(open(prefix + "_kSpider_pairwise.tsv"))[1:] if l.strip())]


def _n_names(prefix):
    return len([l for l in list(open(prefix + ".namesMap"))[1:] if l.strip()])


def _cut_both_ways(prefix, dist, cutoff):
    """(bytes from the tree file, bytes of the oracle over the full TSV); the two share a file name."""
    path = ref_cluster.output_path(prefix, cutoff)
    engine.cluster_from_tree(prefix, dist, cutoff)
    got = _read(path)
    os.remove(path)
    assert _read(ref_cluster.write_clusters(prefix, dist, cutoff)) == got, (dist, cutoff)
    os.remove(path)
    return got


def _cutoffs_around(texts):
    out = {0.0, 1.0}
    for t in texts:
        v = float(t)
        if v == v and 0.0 <= v <= 1.0:
            out.update(c for c in (v, float(np.nextafter(v, 2.0)), float(np.nextafter(v, -1.0))) if 0.0 <= c <= 1.0)
    return sorted(out)


@pytest.mark.parametrize("tag", ["setA", "setB"])
def test_cut_of_the_tree_equals_the_cluster_file(tag, tmp_path):
    shutil.copytree(os.path.join(GOLD, tag), tmp_path / tag)
    prefix = str(tmp_path / tag / "sigs")
    n = _n_names(prefix)
    for dist, col in DISTS.items():
        rows = _rows(prefix, col)
        tree = tr.tree_rows(n, rows)
        with open(prefix + f"_kSpider_tree_{dist}.tsv", "w") as f:
            f.write(tr.tree_tsv(dist, n, rows))
        distinct = set()
        for c in _cutoffs_around({r[2] for r in tree}):
            distinct.add(_cut_both_ways(prefix, dist, c))
        assert len(distinct) >= 3, (tag, dist)                       # the cut-offs do tell clusterings apart
        assert len(tree) == n - len(ref_cluster.clusters(prefix, dist, 0.0))
        assert max(r[3] for r in tree) == max(len(c) for c in ref_cluster.clusters(prefix, dist, 0.0))
    assert not glob.glob(str(tmp_path / tag / "*.partial"))


def _write_prefix(prefix, n, rows):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n" + "".join(f"{i + 1} g{i + 1}\n" for i in range(n)))
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n" + "".join(f"{i + 1}\t{i + 1}\t10\n" for i in range(n)))
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write("source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n")
        f.write("".join(f"{a}\t{b}\t1\t{t}\t{t}\t{t}\n" for a, b, t in rows))


def test_nan_and_inf_rows_repeats_and_ties(tmp_path):
    """A NaN row is kept at every cut-off and an inf row at every cut-off of [0, 1]; equal texts, "0.5" beside "0.50", a repeated
    pair with two values and a self pair."""
    prefix = str(tmp_path / "t")
    rows = [(1, 2, "0.5"), (2, 3, "0.50"), (1, 3, "0.5"), (3, 4, "nan"), (4, 5, "inf"), (5, 6, "0.25"), (5, 6, "0.75"), (6, 6, "1"),
            (7, 8, "0"), (1, 9, "0.1"), (2, 9, "0.1")]
    _write_prefix(prefix, 9, rows)
    tree = tr.tree_rows(9, rows)
    assert [r[:3] for r in tree] == [(3, 4, "nan"), (4, 5, "inf"), (5, 6, "0.75"), (1, 2, "0.5"), (2, 3, "0.50"), (1, 9, "0.1"), (7, 8, "0")]
    assert [r[3] for r in tree] == [2, 3, 4, 2, 6, 7, 2]
    with open(prefix + "_kSpider_tree_max_cont.tsv", "w") as f:
        f.write(tr.tree_tsv("max_cont", 9, rows))
    for c in _cutoffs_around(["0.5", "0.25", "0.75", "0.1"]):
        _cut_both_ways(prefix, "max_cont", c)
    assert _cut_both_ways(prefix, "max_cont", 1.0) == b"g1\ng2\ng3,g4,g5\ng6\ng7\ng8\ng9\n"
    assert not glob.glob(str(tmp_path / "*.partial"))


def test_refusals_leave_nothing_behind(tmp_path):
    prefix = str(tmp_path / "t")
    _write_prefix(prefix, 4, [(1, 2, "0.5")])
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_from_tree(prefix, "max_cont", 0.3)              # no tree file
    assert ei.value.code == engine.KSP_E_IO and "_kSpider_tree_max_cont.tsv" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_from_tree(prefix, "jaccard", 0.3)
    assert ei.value.code == engine.KSP_E_ARG
    assert sorted(os.listdir(tmp_path)) == before
    tree = prefix + "_kSpider_tree_max_cont.tsv"
    for body in ("1\t5\t0.5\t2\n", "0\t2\t0.5\t2\n", "1\t2\tx\t2\n", "1\t2\n"):          # an id .namesMap does not have (also below the cut), a bad value, a short row
        with open(tree, "w") as f:
            f.write("source_1\tsource_2\tmax_cont\tmerged_size\n" + body)
        for c in (0.3, 0.9):
            with pytest.raises(engine.KspError) as ei:
                engine.cluster_from_tree(prefix, "max_cont", c)
            assert ei.value.code == engine.KSP_E_IO, body
    os.remove(tree)
    assert sorted(os.listdir(tmp_path)) == before
    L = engine.lib()
    assert L.kspider_cluster_from_tree(None, b"max_cont", 0.5) == engine.KSP_E_ARG
    assert L.kspider_tree(None, b"max_cont", 0) == engine.KSP_E_ARG
    assert L.kspider_pairwise_and_tree(None, 1, b"max_cont", 0) == engine.KSP_E_ARG


def test_argument_checks_need_no_device(tmp_path):
    prefix = str(tmp_path / "nope")
    with pytest.raises(engine.KspError) as ei:
        engine.tree(prefix, "jaccard")
    assert ei.value.code == engine.KSP_E_ARG
    for dist in ("jaccard", "ani"):
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_and_tree(prefix, 1, dist)
        assert ei.value.code == engine.KSP_E_ARG and dist in str(ei.value)
    for col in (2, 6):
        with pytest.raises(engine.KspError) as ei:
            engine.edges_forest(4, 0, 0, 0, col)
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.edges_forest(4, 0, 5, 0, 5)                              # NULL pointers with edges
    assert ei.value.code == engine.KSP_E_ARG
    z = np.zeros(1, dtype=np.uint32)
    with pytest.raises(engine.KspError) as ei:
        engine.forest_ranked(4, z, np.array([4], dtype=np.uint32), z)   # a node out of range
    assert ei.value.code == engine.KSP_E_ARG and "out of range" in str(ei.value)
    L = engine.lib()
    n = ctypes.c_uint32(7)
    assert L.ksp_forest_ranked(0, 4, None, None, None, 3, z.ctypes.data, ctypes.byref(n)) == engine.KSP_E_ARG
    assert L.ksp_forest_ranked(0, 4, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, None, ctypes.byref(n)) == engine.KSP_E_ARG
    assert L.ksp_forest_ranked(0, 4, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, None) == engine.KSP_E_ARG
    assert L.ksp_edges_forest(0, 4, None, 0, None, 5, None, None) == engine.KSP_E_ARG
    assert L.ksp_edges_forest(0, 4, z.ctypes.data, 2**32 - 1, z.ctypes.data, 5, z.ctypes.data, ctypes.byref(n)) == engine.KSP_E_LIMIT
    assert n.value == 7 and not list(tmp_path.iterdir())


def test_constants_are_mirrored_and_exported():
    text = open(os.path.join(ROOT, "include", "kspider_amd.h")).read()
    assert int(re.search(r"#define KSP_TREE_CHUNK_EDGES (\d+)u", text).group(1)) == engine.TREE_CHUNK_EDGES
    import kspider_amd
    assert kspider_amd.tree is engine.tree and kspider_amd.cluster_from_tree is engine.cluster_from_tree
    assert kspider_amd.pairwise_and_tree is engine.pairwise_and_tree


def test_restatement_order_and_unique_forest():
    """Kruskal of the restatement: key descending, a NaN on top, lower index first among equals; self pairs never merge."""
    e = np.zeros(7, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = [0, 1, 0, 2, 3, 3, 4], [1, 2, 2, 3, 3, 5, 5], [5, 5, 5, 0, 9, 2, 0]
    cnt = np.array([10, 10, 10, 10, 10, 0])
    k = tr.keys(e, cnt, 5)
    assert k[6] == tr.NAN_KEY and k[5] == 0x7F800000 and k[3] == 0 and k[0] == k[1] == k[2]      # 0 / 0, 2 / 0, 0 / 10
    assert tr.forest(6, e, cnt, 5).tolist() == [6, 5, 0, 1, 3]
    assert tr.kruskal(3, [0, 0], [1, 1], [4, 9]).tolist() == [1]


def test_restatement_against_scipy_single_linkage():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(21)
    n = 9
    rows, dist = [], []
    thousandths = iter(rng.permutation(999)[:n * (n - 1) // 2] + 1)      # distinct values: with ties the sizes depend on the order of equal merges
    for i in range(n):
        for j in range(i + 1, n):
            v = float(np.float32(next(thousandths) / 1000))
            rows.append((i + 1, j + 1, engine.format_float(v)))
            dist.append(1.0 - float(rows[-1][2]))
    tree = tr.tree_rows(n, rows)
    Z = hierarchy.linkage(np.array(dist), "single")
    assert len(tree) == n - 1
    assert np.allclose([1.0 - float(r[2]) for r in tree], Z[:, 2], rtol=0, atol=1e-12)
    assert sorted(r[3] for r in tree) == sorted(int(s) for s in Z[:, 3])


def test_newick_parser_of_the_tests():
    leaves, lengths = tr.parse_newick("((a:0.25,b:0.25):0.5,(c:0.1,(d:0.05,e:0.05):0.05):0.65);\n")
    assert set(leaves) == set("abcde") and all(abs(d - 0.75) < 1e-12 for d in leaves.values()) and len(lengths) == 8
    assert tr.parse_newick("x;\n") == ({"x": 0.0}, [])

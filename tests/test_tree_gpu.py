"""The single-linkage tree on the GPU against the restatement in tests/tree_restate.py.  The order of edges is
strict, so the maximum spanning forest is unique and the device's record indices are compared with Kruskal's element for
element — through both device entries: ksp_edges_forest over ksp_edge records in device memory and ksp_forest_ranked over host
edges with the same keys as ranks.  Shapes where Boruvka goes wrong (mutual picks, ties, hook chains, stars, repeats, self pairs,
NaN / inf), the sizes where a ballot and a chunk begin and end, a grid so small that every workgroup loops, a contended giant
component, the join's own records cut at 12 cut-offs against ksp_components_edges, and the file-writing calls against
kspider_cluster and oracle.ref_cluster.  Every output has sentinels behind it and d_edges is compared after every call."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import cut_restate as cr
import sweep_restate as sr
import tree_restate as tr
from kspider_amd import engine
from oracle import ref_cluster

pytestmark = pytest.mark.gpu

C = engine.TREE_CHUNK_EDGES
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "cluster_tree")
TAIL = 7                        # sentinel entries behind the last one h_index could hold
FILL = 0xDEADBEEF
COUNT = 1 << 20                 # k-mers of every source of the shape cases: shared / COUNT is exact, and the value of all three columns


def _edges(s1, s2, shared):
    e = np.zeros(len(s1), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = s1, s2, shared
    return e


def _check(n_nodes, edges, cnt, cols=(5,)):
    """Both device entries against the restatement, index for index; returns the forest of the last column."""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    n = len(edges)
    ed = engine.DeviceBuffer.from_numpy(edges) if n else None
    cd = engine.DeviceBuffer.from_numpy(cnt)
    try:
        for col in cols:
            key = tr.keys(edges, cnt, col)
            want = tr.kruskal(n_nodes, edges["source_1"], edges["source_2"], key)
            got = engine.edges_forest(n_nodes, ed.ptr.value if ed else 0, n, cd.ptr.value, col, tail=TAIL, fill=FILL)
            assert got.tolist() == want.tolist(), ("ksp_edges_forest", col, n)
            if n:
                assert (ed.to_numpy(engine.EDGE_DTYPE, n) == edges).all(), "d_edges was written"
            rank = np.unique(key, return_inverse=True)[1].reshape(-1) if n else np.zeros(0, dtype=np.uint32)
            got = engine.forest_ranked(n_nodes, edges["source_1"], edges["source_2"], rank, tail=TAIL, fill=FILL)
            assert got.tolist() == want.tolist(), ("ksp_forest_ranked", col, n)
        return want
    finally:
        for buf in (ed, cd):
            if buf:
                buf.free()


def _same(n):
    return np.full(n, COUNT, dtype=np.uint32)


# ---- shapes where Boruvka goes wrong -----------------------------------------------------------------------------------------

def test_mutual_pick_triangle_and_cycle_of_equal_weights():
    assert _check(2, _edges([0], [1], [7]), _same(2)).tolist() == [0]                               # both ends pick the one record
    assert _check(3, _edges([0, 1, 0], [1, 2, 2], [5, 5, 5]), _same(3)).tolist() == [0, 1]           # equal weights: the index decides
    assert _check(5, _edges([0, 1, 2, 3, 0], [1, 2, 3, 4, 4], [9] * 5), _same(5)).tolist() == [0, 1, 2, 3]
    assert _check(5, _edges([0, 0, 3, 2, 1], [4, 1, 4, 3, 2], [9] * 5), _same(5)).tolist() == [0, 1, 2, 3]   # the cycle in another record order


def test_paths_hook_whole_chains():
    """Strictly increasing weights along a path: every node but the last picks the edge to its right, a chain of 299 hooks made
    in ONE round, which the jump passes must flatten completely; decreasing: the mirror image."""
    n = 300
    i = np.arange(n - 1)
    up = _check(n, _edges(i, i + 1, 1000 + i), _same(n))
    assert up.tolist() == i[::-1].tolist()
    down = _check(n, _edges(i, i + 1, 5000 - i), _same(n))
    assert down.tolist() == i.tolist()
    p = np.random.default_rng(5).permutation(n - 1)
    _check(n, _edges(i[p], i[p] + 1, 1000 + i[p]), _same(n))


def test_star_components_isolated_repeats_and_self_pairs():
    rng = np.random.default_rng(6)
    n = 300
    leaf = np.arange(1, n)
    assert len(_check(n, _edges(np.zeros(n - 1, dtype=int), leaf, rng.integers(1, 50, size=n - 1)), _same(n))) == n - 1   # a star, many equal weights
    assert len(_check(n, _edges(leaf, np.full(n - 1, 0), rng.permutation(n - 1) + 1), _same(n))) == n - 1
    # two components (a 4-cycle, a triangle) and the isolated nodes 7, 8, 9
    got = _check(10, _edges([0, 1, 2, 3, 4, 5, 4], [1, 2, 3, 0, 5, 6, 6], [3, 8, 3, 8, 2, 2, 2]), _same(10))
    assert got.tolist() == [1, 3, 0, 4, 5]
    # a repeated pair with equal values (the lower index wins) and with different values (the larger value wins), in both orders
    assert _check(2, _edges([0, 0, 1], [1, 1, 0], [4, 4, 4]), _same(2)).tolist() == [0]
    assert _check(3, _edges([0, 0, 1, 1], [1, 1, 2, 2], [4, 6, 6, 4]), _same(3)).tolist() == [1, 2]
    # self pairs are skipped, however good: alone, and beside real edges
    assert _check(3, _edges([1, 2], [1, 2], [9, 9]), _same(3)).tolist() == []
    assert _check(3, _edges([1, 0, 2, 1], [1, 1, 2, 2], [90, 3, 80, 2]), _same(3)).tolist() == [1, 3]


def test_nan_inf_and_nothing_shared():
    """Sources 4 and 5 count 0 k-mers: 0 shared with them is a NaN (the top), anything shared an infinite containment (below a
    NaN, above every number).  shared = 0 between sources with k-mers is the value 0: still an edge."""
    cnt = np.array([COUNT, COUNT, COUNT, COUNT, 0, 0, COUNT], dtype=np.uint32)
    e = _edges([0, 1, 2, 3, 0, 4, 2, 0], [1, 2, 3, 4, 4, 5, 6, 3], [COUNT // 2, 0, COUNT // 4, 0, 3, 0, 0, 0])
    for col in (3, 4, 5):
        k = tr.keys(e, cnt, col)
        assert k[5] == tr.NAN_KEY and (k == 0).sum() >= 3
    want = _check(7, e, cnt, cols=(3, 4, 5))
    assert want.tolist()[:2] == [3, 5] and want.tolist()[2] == 4            # column 5: the NaN rows (3-4: max(0 / 0, 0 / n)), then the infinite one
    assert len(want) == 6


def test_the_same_graph_under_three_record_orders():
    rng = np.random.default_rng(7)
    n, m = 400, 3000
    a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    for name, shared in (("distinct", rng.permutation(m) + 1), ("ties", rng.integers(1, 9, size=m))):
        seen = []
        for seed in range(3):
            p = np.random.default_rng(seed).permutation(m)
            e = _edges(a[p], b[p], shared[p])
            f = _check(n, e, _same(n))
            pairs = sorted(zip(np.minimum(e["source_1"][f], e["source_2"][f]).tolist(), np.maximum(e["source_1"][f], e["source_2"][f]).tolist(),
                               e["shared"][f].tolist()))
            seen.append(pairs if name == "distinct" else sorted(s for _, _, s in pairs))
        assert seen[0] == seen[1] == seen[2], name                         # distinct values: the same (pair, value)s; ties: the same values


# ---- sizes -----------------------------------------------------------------------------------------------------------------

N_NODES = 5200


def _random_case(n, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(3000, 4001, size=N_NODES).astype(np.uint32)
    s1, s2 = rng.integers(0, N_NODES, size=n), rng.integers(0, N_NODES, size=n)
    shared = (rng.random(n) * np.minimum(cnt[s1], cnt[s2])).astype(np.uint64)
    return _edges(s1, s2, shared), cnt


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17])
def test_ballot_and_chunk_boundaries(n):
    e, cnt = _random_case(n, 100 + n)
    _check(N_NODES, e, cnt, cols=(3, 4, 5))


def test_every_workgroup_loops_over_chunks(monkeypatch):
    """40 chunks (the last one short) on a grid of 3 workgroups: 13 or 14 chunks each."""
    monkeypatch.setenv("KSP_TREE_MAX_WORKGROUPS", "3")
    e, cnt = _random_case(40 * C - 5, 40)
    f = _check(N_NODES, e, cnt, cols=(3, 4, 5))
    assert len(f) > 5000


def test_contended_giant_component():
    """One component of 5 000 nodes with 3 x 10^5 random edges: after two or three rounds every offer goes to a few labels."""
    rng = np.random.default_rng(9)
    n, m = 5000, 300000
    cnt = rng.integers(3000, 4001, size=n).astype(np.uint32)
    s1, s2 = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    e = _edges(s1, s2, (rng.random(m) * np.minimum(cnt[s1], cnt[s2])).astype(np.uint64))
    assert len(_check(n, e, cnt)) == n - 1


# ---- the join's own records --------------------------------------------------------------------------------------------------

def test_cuts_of_the_forest_equal_the_components_of_all_records():
    """The 3 000-source join of tests/test_sweep_gpu.py through ksp_edges_forest: at 12 cut-offs — printed values of rows, the
    floats next to them, 0 and 1 — a union-find over the forest's kept records gives the labels ksp_components_edges gives on
    ALL records."""
    from kspider_amd import synth
    sk = synth.generate("C2", n_sources=3000, mean_size=400, cluster_cap=60, seed=99)
    keys_d = engine.DeviceBuffer.from_numpy(sk.keys)
    cnt_d = engine.DeviceBuffer.from_numpy(sk.sizes.astype(np.uint32))
    eng = engine.Engine(0)
    eng.build_blocks(keys_d.ptr.value, sk.offsets)
    cap = int(eng.edge_bound(0, eng.num_tiles)) + 1
    ed = engine.DeviceBuffer(cap * 16)
    m = eng.join(0, eng.num_tiles, ed.ptr.value, cap)
    ev = ed.to_numpy(engine.EDGE_DTYPE, m)
    assert m > C
    for col in (3, 4, 5):
        f = engine.edges_forest(sk.n_sources, ed.ptr.value, m, cnt_d.ptr.value, col, tail=TAIL, fill=FILL)
        assert f.tolist() == tr.forest(sk.n_sources, ev, sk.sizes, col).tolist(), col
        fe = ev[f]
        texts = sr.column_texts(fe, sk.sizes, col)
        by_value = sorted(set(texts), key=float)
        cutoffs = [0.0, 1.0]
        for q in (1, 2, 3, 4, 5):
            v = float(by_value[len(by_value) * q // 6])
            cutoffs += [v, float(np.nextafter(v, 2.0))] if q % 2 else [v, float(np.nextafter(v, -1.0))]
        assert len(cutoffs) == 12
        sizes = set()
        for c in cutoffs:
            keep = np.array([cr.keep(t, c) for t in texts], dtype=bool)
            mine = sr.union_find(sk.n_sources, fe["source_1"][keep], fe["source_2"][keep])
            full = engine.components_edges(sk.n_sources, ed.ptr.value, m, cnt_d.ptr.value, col, c)
            assert (mine == full).all(), (col, c)
            sizes.add(len(np.unique(mine)))
        assert len(sizes) >= 6, col
    assert (ed.to_numpy(engine.EDGE_DTYPE, m) == ev).all()
    eng.close()
    for buf in (keys_d, cnt_d, ed):
        buf.free()


# ---- files -------------------------------------------------------------------------------------------------------------------

DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _tree_rows(prefix, dist):
    lines = _read(prefix + f"_kSpider_tree_{dist}.tsv").decode().split("\n")
    assert lines[0] == f"source_1\tsource_2\t{dist}\tmerged_size" and lines[-1] == ""
    return [l.split("\t") for l in lines[1:-1]]


def _check_newick(prefix, dist, n, rows, n_clusters):
    leaves, lengths = tr.parse_newick(_read(prefix + f"_kSpider_tree_{dist}.newick").decode())
    assert set(leaves) == {f"genome_{i + 1}" for i in range(n)}
    assert all(x >= 0 for x in lengths)
    root = 1.0 if n_clusters > 1 else min(1.0, max(0.0, 1.0 - min(float(r[2]) for r in rows)))
    tol = 5e-7 * n                                                        # "%.6g" per branch (heights are at most 1), at most n branches on a path
    assert all(abs(d - root) <= tol for d in leaves.values()), (dist, root)
    sizes = [int(r[3]) for r in rows]
    assert all(2 <= s <= n for s in sizes)


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The 400-source index of tests/test_sweep_gpu.py, the TSVs of engine.pairwise, and per distance 8 cut-offs — 0, 1, three
    printed values of rows and the floats next to them — with what kspider_cluster writes for each over the full TSV."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("tree")
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    (d / "index").mkdir()
    index = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(index, sk.keys, sk.offsets)
    _names_map(index, sk.n_sources)
    shutil.copytree(d / "index", d / "full")
    prefix = str(d / "full" / "ix")
    engine.pairwise(prefix, 2)
    tsv, seq = _read(prefix + "_kSpider_pairwise.tsv"), _read(prefix + "_kSpider_seqToKmersNo.tsv")
    rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
    cutoffs, want, n_clusters = {}, {}, {}
    for dist, col in DISTS.items():
        distinct = sorted({r[col] for r in rows}, key=float)
        picks = [float(distinct[len(distinct) * q // 4]) for q in (1, 2, 3)]
        cutoffs[dist] = [0.0, 1.0] + picks + [float(np.nextafter(picks[0], 2.0)), float(np.nextafter(picks[1], -1.0)), float(np.nextafter(picks[2], 2.0))]
        for c in cutoffs[dist]:
            engine.cluster(prefix, dist, c)
            path = ref_cluster.output_path(prefix, c)
            want[dist, c] = _read(path)
            os.remove(path)
            assert want[dist, c] == _read(ref_cluster.write_clusters(prefix, dist, c))
            os.remove(path)
        n_clusters[dist] = want[dist, 0.0].count(b"\n")
        assert len({want[dist, c] for c in cutoffs[dist]}) >= 4
    return dict(dir=d, prefix=prefix, tsv=tsv, seq=seq, rows=rows, cutoffs=cutoffs, want=want, n=sk.n_sources, n_clusters=n_clusters)


def _check_cuts(full, prefix, dist):
    for c in full["cutoffs"][dist]:
        engine.cluster_from_tree(prefix, dist, c)
        path = ref_cluster.output_path(prefix, c)
        got = _read(path)
        os.remove(path)
        assert got == full["want"][dist, c], (dist, c)


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_tree_files(full, monkeypatch, devices):
    """The guarantee of DESIGN.md §7f: the cut of the tree equals kspider_cluster, from the tree kspider_tree reads off the TSV and
    from the one kspider_pairwise_and_tree takes from HBM."""
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    n = full["n"]
    for dist, col in DISTS.items():
        d = full["dir"] / f"file_{dist}_{devices}"
        shutil.copytree(full["dir"] / "full", d)
        on_file = str(d / "ix")
        before = set(os.listdir(d))
        engine.tree(on_file, dist, True)
        assert set(os.listdir(d)) - before == {f"ix_kSpider_tree_{dist}.tsv", f"ix_kSpider_tree_{dist}.newick"}
        d2 = full["dir"] / f"fused_{dist}_{devices}"
        shutil.copytree(full["dir"] / "index", d2)
        fused = str(d2 / "ix")
        engine.pairwise_and_tree(fused, 2, dist, True)
        assert _read(fused + "_kSpider_pairwise.tsv") == full["tsv"] and _read(fused + "_kSpider_seqToKmersNo.tsv") == full["seq"], (dist, devices)
        assert not glob.glob(str(d / "*.partial")) and not glob.glob(str(d2 / "*.partial"))
        rows_file, rows_fused = _tree_rows(on_file, dist), _tree_rows(fused, dist)
        assert len(rows_file) == len(rows_fused) == n - full["n_clusters"][dist]
        assert sorted(r[2] for r in rows_file) == sorted(r[2] for r in rows_fused)
        # the file's own tree equals the restatement's, byte for byte (same order, same ties, same sizes)
        assert _read(on_file + f"_kSpider_tree_{dist}.tsv").decode() == tr.tree_tsv(dist, n, [(int(r[0]), int(r[1]), r[col]) for r in full["rows"]])
        for prefix, rows in ((on_file, rows_file), (fused, rows_fused)):
            vals = [tr.weight_key(r[2]) for r in rows]
            assert vals == sorted(vals)
            _check_newick(prefix, dist, n, rows, full["n_clusters"][dist])
            _check_cuts(full, prefix, dist)


def test_exe_and_refusals(full):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    before = sorted(os.listdir(d))
    for call in (lambda: engine.pairwise_and_tree(prefix, 1, "ani"), lambda: engine.tree(prefix, "jaccard"), lambda: engine.pairwise_and_tree(prefix, 1, "jaccard"),
                 lambda: engine.edges_forest(4, 0, 5, 0, 5), lambda: engine.edges_forest(4, 0, 0, 0, 6)):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.tree(prefix, "ani")                                       # ANI without its column file, as kspider_cluster refuses it
    assert "ani_col" in str(ei.value)
    assert sorted(os.listdir(d)) == before
    c1, c2 = full["cutoffs"]["max_cont"][2], full["cutoffs"]["max_cont"][4]
    run = subprocess.run([EXE, prefix, "max_cont", "--newick", "--cut", repr(c1), "--cut", repr(c2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    for c in (c1, c2):
        assert _read(ref_cluster.output_path(prefix, c)) == full["want"]["max_cont", c]
    assert os.path.exists(prefix + "_kSpider_tree_max_cont.newick") and not glob.glob(str(d / "*.partial"))
    run = subprocess.run([EXE, prefix, "jaccard"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"jaccard" in run.stderr
    # a namesMap that does not cover the nodes: refused like kspider_cluster, and nothing new is left behind
    for path in glob.glob(prefix + "_kSpider_tree*") + glob.glob(prefix + "_kSpider_clusters*"):
        os.remove(path)
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.tree(prefix, "max_cont", True)
    assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(d)) == before


def test_ani_on_the_file_path(full):
    d = full["dir"] / "ani"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    engine.estimate_ani(prefix, 2, 1000)
    vals = sorted({float(v) for v in _read(prefix + "_kSpider_pairwise.ani_col.tsv").decode().split("\n")[1:-1]})
    engine.tree(prefix, "ani", True)
    for c in (0.0, 1.0, vals[len(vals) // 2], float(np.nextafter(vals[len(vals) // 2], 2.0)), vals[len(vals) // 4]):
        path = ref_cluster.output_path(prefix, c)
        engine.cluster_from_tree(prefix, "ani", c)
        got = _read(path)
        os.remove(path)
        assert got == _read(ref_cluster.write_clusters(prefix, "ani", c)), c
        os.remove(path)


def test_zero_weight_colours(oracle_lib, tmp_path):
    """Rows that exist only with shared_kmers = 0 are united in on the host after the device's forest.  Colours: {1, 2} weight 7;
    {3, 4} weight 0 (the pair shares nothing else); {5, 6} weight 0 AND {5, 6} weight 1 (an ordinary row)."""
    co = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
    src = np.array([1, 2, 3, 4, 5, 6, 5, 6], dtype=np.uint32)
    w = np.array([7, 0, 0, 1], dtype=np.uint32)
    ids = np.arange(1, 7, dtype=np.uint32)
    for sub, counts in (("plain", [10, 20, 30, 40, 50, 60]), ("nan", [10, 20, 30, 0, 50, 60])):      # nan: the row 3-4 is a NaN row, the top of the tree
        d = tmp_path / sub
        d.mkdir()
        prefix = str(d / "z")
        oracle_lib.write_index(prefix, co, src, w, ids, np.array(counts))
        _names_map(prefix, 6)
        engine.pairwise(prefix, 1)
        tsv = _read(prefix + "_kSpider_pairwise.tsv")
        rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
        assert any(r[:3] == ["3", "4", "0"] for r in rows)
        os.remove(prefix + "_kSpider_pairwise.tsv")
        engine.pairwise_and_tree(prefix, 1, "max_cont", True)
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
        fused = _read(prefix + "_kSpider_tree_max_cont.tsv")
        assert fused.decode() == tr.tree_tsv("max_cont", 6, [(int(r[0]), int(r[1]), r[5]) for r in rows]), sub
        tree_rows = _tree_rows(prefix, "max_cont")
        assert [r[:2] for r in tree_rows].count(["3", "4"]) == 1 and (tree_rows[0][:3] == ["3", "4", "-nan"] or tree_rows[0][:3] == ["3", "4", "nan"]) == (sub == "nan")
        _check_newick(prefix, "max_cont", 6, tree_rows, 3)
        engine.tree(prefix, "max_cont", False)
        assert _read(prefix + "_kSpider_tree_max_cont.tsv") == fused
        for c in (0.0, -1.0, 0.02, 0.5, 1.0):
            path = ref_cluster.output_path(prefix, c)
            engine.cluster_from_tree(prefix, "max_cont", c)
            got = _read(path)
            os.remove(path)
            assert got == _read(ref_cluster.write_clusters(prefix, "max_cont", c)), (sub, c)
            os.remove(path)

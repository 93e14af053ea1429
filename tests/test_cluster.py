"""Clustering: `kSpider cluster` = threshold the pairwise TSV + connected components
(/root/reference/pykSpider/kSpider2/ks_clustering.py:63-137).

CPU: the oracle's restatement against the golden cluster files that the REFERENCE's own Clusters class wrote
(tests/golden/make_cluster_golden.py), compared as sets of components — the golden files carry the stand-in's
order, not rustworkx's.  GPU: kspider_cluster() (components on the device) against the oracle byte for byte
(both use the canonical order) and against the golden sets; ksp_components() against a union-find on graphs
with long chains, stars, isolated nodes and a million nodes."""
import os
import shutil

import numpy as np
import pytest

from oracle import ref_cluster

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "clusters")
CASES = [("max_cont", 0.0), ("max_cont", 0.3), ("avg_cont", 0.25), ("min_cont", 0.07), ("min_cont", 0.5), ("max_cont", 1.0)]


def _as_sets(path):
    return sorted(tuple(sorted(l.rstrip("\n").split(","))) for l in open(path) if l.strip())


def _stage(tag, tmp_path):
    d = tmp_path / tag
    shutil.copytree(os.path.join(GOLD, tag), d)
    return str(d / "sigs")


@pytest.mark.parametrize("tag", ["setA", "setB"])
def test_oracle_matches_reference_clusters(tag, tmp_path):
    prefix = _stage(tag, tmp_path)
    for dist, cutoff in CASES:
        out = ref_cluster.write_clusters(prefix, dist, cutoff)
        # the reference names the file with the Python repr of cutoff * 100 (0.07 -> 7.000000000000001)
        assert os.path.basename(out) == f"sigs_kSpider_clusters_{float(cutoff) * 100}%.tsv"
        want = _as_sets(os.path.join(GOLD, tag, f"ref_{dist}_{cutoff}.clusters"))
        assert _as_sets(out) == want, (tag, dist, cutoff)
        names = [n for comp in want for n in comp]
        n_nodes = int(open(prefix + ".namesMap").readline())
        assert len(names) == len(set(names)) == n_nodes   # every node in exactly one component, singletons included
        os.remove(out)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["setA", "setB"])
def test_gpu_clusters_equal_oracle_and_reference(tag, tmp_path):
    from kspider_amd import engine
    prefix = _stage(tag, tmp_path)
    for dist, cutoff in CASES:
        want_path = ref_cluster.write_clusters(prefix, dist, cutoff)
        want = open(want_path, "rb").read()
        os.remove(want_path)
        engine.cluster(prefix, dist, cutoff)
        assert os.path.exists(want_path), "file name differs from the reference's"
        assert open(want_path, "rb").read() == want
        assert _as_sets(want_path) == _as_sets(os.path.join(GOLD, tag, f"ref_{dist}_{cutoff}.clusters"))
        assert not os.path.exists(want_path + ".partial")
        os.remove(want_path)


@pytest.mark.gpu
def test_gpu_cluster_after_gpu_pairwise_and_loud_failures(oracle_lib, tmp_path):
    """index -> kspider_pairwise (HIP) -> kspider_cluster (HIP), against the oracle's pairwise + clustering."""
    from kspider_amd import engine, synth
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    prefix = str(tmp_path / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{sk.n_sources}\n")
        for i in range(sk.n_sources):
            f.write(f"{i + 1} genome_{i + 1}\n")
    engine.pairwise(prefix, 2)
    for dist, cutoff in (("max_cont", 0.2), ("min_cont", 0.05), ("avg_cont", 0.6)):
        engine.cluster(prefix, dist, cutoff)
        got = open(ref_cluster.output_path(prefix, cutoff), "rb").read()
        os.remove(ref_cluster.output_path(prefix, cutoff))
        assert got == open(ref_cluster.write_clusters(prefix, dist, cutoff), "rb").read()
        assert 1 < got.count(b"\n") < sk.n_sources
    # failures are loud: unknown distance, ANI without its file, a namesMap that does not cover the nodes
    with pytest.raises(engine.KspError):
        engine.cluster(prefix, "jaccard", 0.1)
    with pytest.raises(engine.KspError) as ei:
        engine.cluster(prefix, "ani", 0.1)
    assert "ani_col" in str(ei.value)
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    with pytest.raises(engine.KspError) as ei:
        engine.cluster(prefix, "max_cont", 0.0)
    assert ei.value.code == engine.KSP_E_IO


def _union_find(n, a, b):
    parent = np.arange(n)
    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(a.tolist(), b.tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n)], dtype=np.uint32)


@pytest.mark.gpu
def test_components_kernel():
    from kspider_amd import engine
    rng = np.random.default_rng(5)
    # no edges, no nodes
    assert engine.components(0, np.zeros(0, np.uint32), np.zeros(0, np.uint32)).size == 0
    assert (engine.components(7, np.zeros(0, np.uint32), np.zeros(0, np.uint32)) == np.arange(7)).all()
    # a 50 000-node chain given in shuffled order (deep trees), a star, self loops, duplicate edges, isolated nodes
    n = 60_000
    chain = np.arange(50_000, dtype=np.uint32)
    a = np.concatenate([chain[:-1], np.full(3000, 50_010, np.uint32), [7, 7, 9]]).astype(np.uint32)
    b = np.concatenate([chain[1:], np.arange(52_000, 55_000, dtype=np.uint32), [7, 8, 9]]).astype(np.uint32)
    p = rng.permutation(a.size)
    lab = engine.components(n, a[p], b[p])
    assert (lab == _union_find(n, a, b)).all()
    assert (lab[:50_000] == 0).all() and lab[59_999] == 59_999
    # random sparse graph, 200 000 nodes
    n = 200_000
    a = rng.integers(0, n, size=150_000, dtype=np.uint32)
    b = rng.integers(0, n, size=150_000, dtype=np.uint32)
    assert (engine.components(n, a, b) == _union_find(n, a, b)).all()
    # an index beyond the node count is refused
    with pytest.raises(engine.KspError):
        engine.components(5, np.array([1], np.uint32), np.array([5], np.uint32))
    # 2 M nodes, 6 M edges in clusters: labels are the smallest member, consistent along every edge
    n = 2_000_000
    grp = rng.integers(0, 50_000, size=n)
    order = np.argsort(grp, kind="stable")
    a = order[:-1].astype(np.uint32)
    b = order[1:].astype(np.uint32)
    same = grp[a] == grp[b]
    a, b = a[same], b[same]
    extra = rng.integers(0, a.size, size=4_000_000)
    a2, b2 = np.concatenate([a, a[extra]]), np.concatenate([b, b[np.roll(extra, 1)]])
    keep = grp[a2] == grp[b2]
    lab = engine.components(n, a2[keep], b2[keep])
    first = np.full(50_000, n, dtype=np.int64)
    np.minimum.at(first, grp, np.arange(n))
    assert (lab == first[grp]).all()


def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("n,mean,cap", [(400, 300, 25), (20000, 300, 150)])
def test_pairwise_and_cluster_from_hbm_equals_the_two_calls(oracle_lib, tmp_path, n, mean, cap):
    """kspider_pairwise_and_cluster (components from the join's edge records while they are in HBM) writes the pairwise
    TSV of kspider_pairwise and the cluster file kspider_cluster derives from that TSV, byte for byte — and the
    oracle's restatement of ks_clustering.py agrees.  Cut-offs include values that ARE printed containments of rows
    (the test `text -> float -> x 100 not below cutoff x 100` decided on the device by one critical float), 0 and 1."""
    from kspider_amd import engine, synth
    sk = synth.generate("C2", n_sources=n, mean_size=mean, cluster_cap=cap, seed=4321 + n)
    prefix = str(tmp_path / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    _names_map(prefix, sk.n_sources)
    engine.pairwise(prefix, 2)
    tsv = open(prefix + "_kSpider_pairwise.tsv", "rb").read()
    rows = tsv.decode().splitlines()[1:]
    assert len(rows) > (100 if n < 1000 else 500_000)
    pick = [rows[len(rows) // 3].split("\t"), rows[2 * len(rows) // 3].split("\t")]
    cases = [("max_cont", 0.2), ("min_cont", 0.05), ("avg_cont", 0.6), ("max_cont", 0.0), ("min_cont", 1.0),
             ("max_cont", float(pick[0][5])), ("min_cont", float(pick[1][3])), ("avg_cont", float(pick[0][4]))]
    if n > 1000:
        cases = cases[:2] + cases[5:]
    for dist, cutoff in cases:
        engine.cluster(prefix, dist, cutoff)
        path = ref_cluster.output_path(prefix, cutoff)
        want = open(path, "rb").read()
        os.remove(path)
        os.remove(prefix + "_kSpider_pairwise.tsv")
        engine.pairwise_and_cluster(prefix, 2, dist, cutoff)
        assert open(prefix + "_kSpider_pairwise.tsv", "rb").read() == tsv
        got = open(path, "rb").read()
        assert got == want, (dist, cutoff)
        if n < 1000:
            os.remove(path)
            assert got == open(ref_cluster.write_clusters(prefix, dist, cutoff), "rb").read()
        os.remove(path)
    with pytest.raises(engine.KspError):
        engine.pairwise_and_cluster(prefix, 1, "ani", 0.5)
    with pytest.raises(engine.KspError):
        engine.pairwise_and_cluster(prefix, 1, "jaccard", 0.5)


@pytest.mark.gpu
def test_components_over_device_edge_records():
    """ksp_components_edges on the edges ksp_engine_join left in device memory, against a union-find over the rows the
    reference's test keeps (float32 maths of the TSV writer, '%g' text, Python float x 100 not below cutoff x 100)."""
    from kspider_amd import engine, synth
    sk = synth.generate("C2", n_sources=3000, mean_size=400, cluster_cap=60, seed=99)
    keys_d = engine.DeviceBuffer.from_numpy(sk.keys)
    cnt_d = engine.DeviceBuffer.from_numpy(sk.sizes.astype(np.uint32))
    eng = engine.Engine(0)
    eng.build_blocks(keys_d.ptr.value, sk.offsets)
    cap = int(eng.edge_bound(0, eng.num_tiles)) + 1
    ed = engine.DeviceBuffer(cap * 16)
    m = eng.join(0, eng.num_tiles, ed.ptr.value, cap)
    ev = ed.to_numpy(engine.EDGE_DTYPE, m)
    n1 = sk.sizes[ev["source_1"]].astype(np.float32)
    n2 = sk.sizes[ev["source_2"]].astype(np.float32)
    sh = ev["shared"].astype(np.float32)
    c12, c21 = sh / n2, sh / n1
    cols = {3: np.minimum(c12, c21), 4: ((c12 + c21).astype(np.float64) / 2.0).astype(np.float32), 5: np.maximum(c12, c21)}
    for col, cutoff in ((5, 0.3), (3, 0.1), (4, 0.5), (5, 0.0), (3, 2.0), (4, float("%g" % cols[4][m // 2]))):
        text = np.array([float("%g" % v) for v in cols[col]])
        keep = ~(text * 100 < cutoff * 100)
        want = _union_find(sk.n_sources, ev["source_1"][keep], ev["source_2"][keep])
        got = engine.components_edges(sk.n_sources, ed.ptr.value, m, cnt_d.ptr.value, col, cutoff)
        assert (got == want).all(), (col, cutoff, int(keep.sum()))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["plain", "nan"])
def test_pairwise_and_cluster_with_rows_of_zero_weight_colours(oracle_lib, tmp_path, sub):
    """A row that exists only with shared_kmers = 0 (the pair 3-4 of tests/zero_weight_inputs.py; a NaN row when source 4 counts
    0 k-mers) is united in on the host after the device's components: the same TSV as kspider_pairwise and the cluster file of
    ks_clustering.py on that TSV, at cut-offs the row passes (0, negative; every one as a NaN) and fails."""
    import zero_weight_inputs
    from kspider_amd import engine
    prefix = str(tmp_path / "z")
    zero_weight_inputs.write(oracle_lib, prefix, sub)
    engine.pairwise(prefix, 1)
    tsv = open(prefix + "_kSpider_pairwise.tsv", "rb").read()
    assert any(r.split("\t")[:3] == ["3", "4", "0"] for r in tsv.decode().split("\n")[1:-1])
    seen = set()
    for dist in ("min_cont", "avg_cont", "max_cont"):
        for cutoff in (0.0, -1.0, 0.02, 0.5, 1.0):
            os.remove(prefix + "_kSpider_pairwise.tsv")
            engine.pairwise_and_cluster(prefix, 1, dist, cutoff)
            assert open(prefix + "_kSpider_pairwise.tsv", "rb").read() == tsv, (sub, dist, cutoff)
            path = ref_cluster.output_path(prefix, cutoff)
            got = open(path, "rb").read()
            os.remove(path)
            assert got == open(ref_cluster.write_clusters(prefix, dist, cutoff), "rb").read(), (sub, dist, cutoff)
            os.remove(path)
            seen.add(got)
    assert len(seen) >= 2

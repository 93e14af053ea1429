"""ANI on the device: ksp_edges_ani against the host's text definition bit for bit, the ANI cut of the components pass,
and the fused calls kspider_pairwise_ani[_and_cluster] against kspider_pairwise + kspider_estimate_ani +
kspider_cluster(prefix, "ani", c) and the Python restatement of ks_pairwise.py (tests/ani_restate.py)."""
import os

import numpy as np
import pytest

from ani_restate import estimate_ani as restated
from oracle import ref_cluster

pytestmark = pytest.mark.gpu
SCALE = 1000


def _union_find(n, a, b):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(v) for v in range(n)], dtype=np.uint32)


def _host_min_max(edges, counts):
    n1 = counts[edges["source_1"]].astype(np.float32)
    n2 = counts[edges["source_2"]].astype(np.float32)
    sh = edges["shared"].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        c12, c21 = sh / n2, sh / n1
    return np.where(c21 < c12, c21, c12), np.where(c12 < c21, c21, c12)   # std::min / std::max


def _edges(rng, n_nodes, m, counts, shared_max):
    from kspider_amd import engine
    a = rng.integers(0, n_nodes, m)
    b = rng.integers(0, n_nodes, m)
    keep = a != b
    a, b = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    ed = np.zeros(a.size, dtype=engine.EDGE_DTYPE)
    ed["source_1"], ed["source_2"] = a, b
    ed["shared"] = rng.integers(1, shared_max + 1, a.size)
    ed["shared"] = np.minimum(ed["shared"], np.maximum(1, np.minimum(counts[a], counts[b])))
    return ed


@pytest.mark.parametrize("k", [1, 21, 31])
def test_edges_ani_equals_host_definition(k):
    from kspider_amd import engine
    rng = np.random.default_rng(k)
    n = 5000
    counts = rng.integers(1, 6000, n).astype(np.uint32)
    counts[:64] = 2 ** rng.integers(0, 12, 64)     # power-of-two counts: ties in the 6-digit rounding
    counts[64:80] = 0                               # shared / 0 = inf
    ed = _edges(rng, n, 400_000, counts, 3000)
    ed[:3000]["source_1"] = rng.integers(0, 32, 3000)
    ed[:3000]["source_2"] = rng.integers(32, 64, 3000)
    ed[:3000]["shared"] = rng.integers(1, 4096, 3000)
    ed[3000:3500]["source_1"] = rng.integers(64, 80, 500)
    ed[3000:3500]["source_2"] = rng.integers(100, n, 500)
    d_ed = engine.DeviceBuffer.from_numpy(ed)
    d_cnt = engine.DeviceBuffer.from_numpy(counts)
    d_ani = engine.DeviceBuffer(ed.size * 8)
    engine.edges_ani(d_ed.ptr.value, ed.size, d_cnt.ptr.value, k, d_ani.ptr.value)
    got = d_ani.to_numpy(np.float64, ed.size)
    mn, mx = _host_min_max(ed, counts)
    assert np.isinf(mx).sum() >= 400
    rc, want = engine.ani_values(mn, mx, k, via_table=False)
    assert rc == 0
    assert (got.view(np.uint64) == want.view(np.uint64)).all()

    # the components pass with the ANI cut, against a union-find over the rows the reference's test keeps
    sub = ed[:150_000]
    d_sub = engine.DeviceBuffer.from_numpy(sub)
    vals = want[:150_000]
    for cutoff in (0.0, 0.5, float(vals[77]), float(vals[1234]), 0.95, 1.0):
        keep = ~(vals * 100.0 < cutoff * 100.0)
        exp = _union_find(n, sub["source_1"][keep], sub["source_2"][keep])
        lab = engine.components_edges_ani(n, d_sub.ptr.value, sub.size, d_cnt.ptr.value, k, cutoff)
        assert (lab == exp).all(), cutoff


def test_edges_ani_nan_is_an_error():
    from kspider_amd import engine
    ed = np.zeros(1000, dtype=engine.EDGE_DTYPE)
    ed["source_1"] = np.arange(1000) % 10
    ed["source_2"] = 10 + np.arange(1000) % 10
    counts = np.zeros(20, dtype=np.uint32)           # 0 shared k-mers of sources with 0 k-mers: 0 / 0
    d_ed = engine.DeviceBuffer.from_numpy(ed)
    d_cnt = engine.DeviceBuffer.from_numpy(counts)
    d_ani = engine.DeviceBuffer(ed.size * 8)
    with pytest.raises(engine.KspError) as ei:
        engine.edges_ani(d_ed.ptr.value, ed.size, d_cnt.ptr.value, 21, d_ani.ptr.value)
    assert ei.value.code == 1
    with pytest.raises(engine.KspError) as ei:
        engine.components_edges_ani(20, d_ed.ptr.value, ed.size, d_cnt.ptr.value, 21, 0.5)
    assert ei.value.code == 1


def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _check_fused(oracle_lib, prefix, n_sources, k, restate):
    from kspider_amd import engine
    _names_map(prefix, n_sources)
    with open(prefix + ".extra", "w") as f:
        f.write(f"{k}\n")
    ani_path = prefix + "_kSpider_pairwise.ani_col.tsv"
    engine.pairwise(prefix, 2)
    tsv = _read(prefix + "_kSpider_pairwise.tsv")
    engine.estimate_ani(prefix, 4, SCALE)
    ani = _read(ani_path)
    assert ani.count(b"\n") == tsv.count(b"\n")
    if restate:
        assert ani == restated(prefix, SCALE)
    os.remove(ani_path)
    os.remove(prefix + "_kSpider_pairwise.tsv")
    engine.pairwise_ani(prefix, 3, SCALE)
    assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
    assert _read(ani_path) == ani
    vals = ani.decode().split("\n")[1:-1]
    cutoffs = [0.0, 0.5, 0.95, 1.0, float(vals[len(vals) // 3]), float(vals[2 * len(vals) // 3])]
    for c in cutoffs:
        engine.cluster(prefix, "ani", c)
        path = ref_cluster.output_path(prefix, c)
        want = _read(path)
        os.remove(path)
        os.remove(ani_path)
        engine.pairwise_ani(prefix, 2, SCALE, c)
        assert _read(path) == want, c
        assert _read(ani_path) == ani
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
        os.remove(path)
    return vals


@pytest.mark.parametrize("devices", [None, "0,0"])
@pytest.mark.parametrize("n,mean,cap,k", [(400, 300, 25, 21), (20000, 300, 150, 31)])
def test_fused_ani_calls_equal_the_separate_calls(oracle_lib, tmp_path, monkeypatch, devices, n, mean, cap, k):
    from kspider_amd import engine, synth
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    sk = synth.generate("C2", n_sources=n, mean_size=mean, cluster_cap=cap, seed=4321 + n)
    prefix = str(tmp_path / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    vals = _check_fused(oracle_lib, prefix, sk.n_sources, k, restate=True)
    assert len(vals) > (100 if n < 1000 else 500_000)
    assert len(set(vals)) > 10
    # the ANI names stay out of the containment-only call
    with pytest.raises(engine.KspError):
        engine.pairwise_and_cluster(prefix, 1, "ani", 0.5)
    with pytest.raises(engine.KspError):
        engine.pairwise_ani(prefix, 1, 0)


def test_fused_ani_full_size_c2(oracle_lib, tmp_path):
    from kspider_amd import synth
    sk = synth.generate("C2")
    prefix = str(tmp_path / "c2")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    vals = _check_fused(oracle_lib, prefix, sk.n_sources, 21, restate=False)
    assert len(vals) > 100_000


def test_weight_zero_colour_rows(oracle_lib, tmp_path):
    """Rows that exist only through weight-0 colours (shared = 0) get their ANI from the host function, in the column and
    in the ANI cut; with a source of 0 k-mers such a row has a NaN containment and the fused call fails before the TSV."""
    from kspider_amd import engine
    co = np.array([0, 2, 5, 7], dtype=np.uint32)
    src = np.array([1, 2, 2, 3, 4, 1, 2], dtype=np.uint32)
    w = np.array([7, 0, 0], dtype=np.uint32)
    prefix = str(tmp_path / "z")
    oracle_lib.write_index(prefix, co, src, w, np.arange(1, 5, dtype=np.uint32), np.array([10, 20, 30, 40]))
    _names_map(prefix, 4)
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    engine.pairwise(prefix, 1)
    tsv = _read(prefix + "_kSpider_pairwise.tsv")
    assert b"\t0\t0\t0\t0\n" in tsv
    engine.estimate_ani(prefix, 1, SCALE)
    ani = _read(prefix + "_kSpider_pairwise.ani_col.tsv")
    assert ani == restated(prefix, SCALE)
    for c in (0.0, 0.3, 1.0):
        engine.cluster(prefix, "ani", c)
        path = ref_cluster.output_path(prefix, c)
        want = _read(path)
        os.remove(path)
        engine.pairwise_ani(prefix, 1, SCALE, c)
        assert _read(path) == want and _read(prefix + "_kSpider_pairwise.ani_col.tsv") == ani
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv

    z = str(tmp_path / "nan")
    oracle_lib.write_index(z, co, src, w, np.arange(1, 5, dtype=np.uint32), np.array([10, 0, 30, 0]))
    with open(z + ".extra", "w") as f:
        f.write("21\n")
    with pytest.raises(engine.KspError):
        engine.pairwise_ani(z, 1, SCALE)
    assert not os.path.exists(z + "_kSpider_pairwise.tsv")
    assert not os.path.exists(z + "_kSpider_pairwise.ani_col.tsv")

"""Every consumer of the join's edge records where counts stop being exact floats: k-mer counts and shared counts above 2^24,
up to 2^32 - 1 and (through the record-taking entry points, which accept any uint64_t) 2^64 - 1, rows that sit exactly on the
critical float of a cut-off or a threshold and on the float before it, forest edges with equal values and values one ulp apart,
NaN and infinite rows, ANI rows on a six-digit tie and next to 0.0001 and 0.9999.  The list is exact_values.hostile_edges, whose
populations tests/test_exact_values_cpu.py counts; that file also shows that the restatements used here equal an exact
(integer) restatement on this list bit for bit, and that a reciprocal-multiply, a conversion through a double, a shared count
narrowed to 32 bits, a truncating conversion, a double division or fminf / fmaxf in the column would each change what these
tests compare.  Every comparison is exact; every output has sentinels behind it where the entry point offers them, and d_edges
is compared after every call.  The drop-in calls run on exact_values.hostile_index against oracle.ref_pairwise and the
restatements over its TSV."""
import functools
import glob
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

import ani_restate
import cut_restate as cr
import derep_restate as dr
import exact_values as xv
import repr_restate as rr
import sweep_restate as sr
import tree_restate as tr
from kspider_amd import engine
from oracle import ref_cluster

pytestmark = pytest.mark.gpu

TAIL = 7
FILL = 0xDEADBEEF
SENTINEL = (0xDEADBEEF, 0xFEEDFACE, 0x0123456789ABCDEF)
DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}
SCALE = 1000


def _sentinels(n):
    e = np.zeros(n, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = SENTINEL
    return e


@pytest.fixture(scope="module")
def dev():
    """The hostile records and counts in device memory, and the list without the rows the ANI calls refuse."""
    h = xv.hostile_edges(1)
    ok = np.ascontiguousarray(h.edges[~h.nan_rows])
    bufs = [engine.DeviceBuffer.from_numpy(h.edges), engine.DeviceBuffer.from_numpy(h.kmer_counts), engine.DeviceBuffer.from_numpy(ok)]
    yield SimpleNamespace(h=h, edges=h.edges, cnt=h.kmer_counts, n=len(h.kmer_counts), m=len(h.edges), ed=bufs[0].ptr.value, cd=bufs[1].ptr.value,
                          ok=ok, okd=bufs[2].ptr.value, bufs=bufs)
    for b in bufs:
        b.free()


def _untouched(dev):
    assert (dev.bufs[0].to_numpy(engine.EDGE_DTYPE, dev.m) == dev.edges).all(), "d_edges was written"
    assert (dev.bufs[2].to_numpy(engine.EDGE_DTYPE, len(dev.ok)) == dev.ok).all(), "d_edges was written"


@functools.lru_cache(maxsize=None)
def _mask(col, cutoff):
    h = xv.hostile_edges(1)
    return cr.edge_mask(h.edges, h.kmer_counts, col, cutoff)


# ---- the cut, the components and the ladder ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("workgroups", [None, "1"])
@pytest.mark.parametrize("col", [3, 4, 5])
def test_cut(dev, monkeypatch, col, workgroups):
    if workgroups:
        monkeypatch.setenv("KSP_CUT_MAX_WORKGROUPS", workgroups)
    for c in dev.h.cutoffs:
        mask = _mask(col, c)
        assert 32 < int(mask.sum()) < dev.m - 32
        out = engine.DeviceBuffer.from_numpy(_sentinels(dev.m + TAIL))
        try:
            kept = engine.edges_cut(dev.ed, dev.m, dev.cd, out.ptr.value, col, c)
            got = out.to_numpy(engine.EDGE_DTYPE, dev.m + TAIL)
        finally:
            out.free()
        assert kept == int(mask.sum()) and (got[:kept] == dev.edges[mask]).all(), (col, c, kept, int(mask.sum()))
        assert (got[kept:] == _sentinels(dev.m + TAIL - kept)).all(), "a record behind n_kept was written"
        _untouched(dev)


@pytest.mark.parametrize("col", [3, 4, 5])
def test_components_and_the_ladder(dev, col):
    want = {c: sr.union_find(dev.n, dev.edges["source_1"][_mask(col, c)], dev.edges["source_2"][_mask(col, c)]) for c in dev.h.cutoffs}
    assert len({w.tobytes() for w in want.values()}) >= 4
    for c in dev.h.cutoffs:
        assert (engine.components_edges(dev.n, dev.ed, dev.m, dev.cd, col, c) == want[c]).all(), (col, c)
        _untouched(dev)
    given = [dev.h.cutoffs[i] for i in np.random.default_rng(col).permutation(len(dev.h.cutoffs))]
    labels, kept = engine.components_edges_sweep(dev.n, dev.ed, dev.m, dev.cd, col, given)
    _untouched(dev)
    for i, c in enumerate(given):
        assert (labels[i] == want[c]).all() and int(kept[i]) == int(_mask(col, c).sum()), (col, c)


# ---- neighbour counts, ranking and dereplication -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [True, False])
def test_degrees_and_ranking(dev, monkeypatch, lds):
    if not lds:
        monkeypatch.setenv("KSP_DEGREE_LDS", "0")
    for col in (3, 4, 5):
        for t in xv.REPR_THRESHOLDS:
            want = rr.degrees(dev.edges, dev.cnt, col, t)
            assert 100 < int(want.sum()) // 2 < dev.m - 100
            assert (engine.edges_degrees(dev.n, dev.ed, dev.m, dev.cd, col, t) == want).all(), (col, t, lds)
            node, count = engine.edges_repr(dev.n, dev.ed, dev.m, dev.cd, col, t)
            assert list(zip(node.tolist(), count.tolist())) == rr.ranked(dict(enumerate(want.tolist()))), (col, t, lds)
            _untouched(dev)


@pytest.mark.parametrize("tail", [True, False])
def test_dereplicate(dev, monkeypatch, tail):
    if not tail:
        monkeypatch.setenv("KSP_DEREP_TAIL", "0")
    for col in (3, 4, 5):
        for t in xv.REPR_THRESHOLDS:
            want = dr.dereplicate(dev.edges, dev.cnt, col, t, dev.n)
            got = engine.edges_dereplicate(dev.n, dev.ed, dev.m, dev.cd, col, t, tail=TAIL, fill=FILL)
            for k in ("rep", "via", "rank", "degree"):
                assert (got[k] == want[k]).all(), (col, t, tail, k)
            assert got["n_reps"] == want["n_reps"]
            _untouched(dev)


# ---- the forest ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", [3, 4, 5])
def test_forest(dev, col):
    key = tr.keys(dev.edges, dev.cnt, col)
    want = tr.kruskal(dev.n, dev.edges["source_1"], dev.edges["source_2"], key)
    got = engine.edges_forest(dev.n, dev.ed, dev.m, dev.cd, col, tail=TAIL, fill=FILL)
    assert got.tolist() == want.tolist(), col
    _untouched(dev)
    rank = np.unique(key, return_inverse=True)[1].reshape(-1)
    got = engine.forest_ranked(dev.n, dev.edges["source_1"], dev.edges["source_2"], rank, tail=TAIL, fill=FILL)
    assert got.tolist() == want.tolist(), col
    # the planted pairs are forest edges: equal values in index order, and the conversion pair in the order a direct conversion gives
    place = {int(e): i for i, e in enumerate(want.tolist())}
    for tag in {t for t in dev.h.tags if t and t[2] == col and t[0] != "ulp"}:
        i, j = [x for x, t in enumerate(dev.h.tags) if t == tag]
        assert place[i] < place[j], tag


# ---- ANI -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ani(k):
    h = xv.hostile_edges(1)
    ok = h.edges[~h.nan_rows]
    mn, mx = xv.as_f32(xv.columns(ok, h.kmer_counts, 3)), xv.as_f32(xv.columns(ok, h.kmer_counts, 5))
    return np.array([ani_restate.ani_of_floats(a, b, k) for a, b in zip(mn.tolist(), mx.tolist())], dtype=np.float64)


@pytest.mark.parametrize("k", [21, 31])
def test_edges_ani(dev, k):
    want = _ani(k)
    assert len(set(want.tolist())) > 1000 and (want == 0.0).any() and (want == 1.0).any()
    out = engine.DeviceBuffer.from_numpy(np.full(len(dev.ok) + TAIL, -7.0))
    try:
        engine.edges_ani(dev.okd, len(dev.ok), dev.cd, k, out.ptr.value)
        got = out.to_numpy(np.float64, len(dev.ok) + TAIL)
    finally:
        out.free()
    assert (got[:len(dev.ok)].view(np.uint64) == want.view(np.uint64)).all(), int((got[:len(dev.ok)] != want).sum())
    assert (got[len(dev.ok):] == -7.0).all()
    _untouched(dev)


def test_components_with_the_ani_cut(dev):
    want = _ani(21)
    mid = sorted(set(want.tolist()))
    for c in (0.5, 0.95, float(repr(mid[len(mid) // 2]))):
        keep = ~(want * 100.0 < c * 100.0)
        assert 16 < int(keep.sum()) < len(keep) - 16                                   # (an ANI below 0.5 is a containment below 5 x 10^-7 at k = 21)
        exp = sr.union_find(dev.n, dev.ok["source_1"][keep], dev.ok["source_2"][keep])
        assert (engine.components_edges_ani(dev.n, dev.okd, len(dev.ok), dev.cd, 21, c) == exp).all(), c
        _untouched(dev)


def test_the_nan_rows_alone_are_refused(dev):
    nan = np.ascontiguousarray(dev.edges[dev.h.nan_rows])
    assert len(nan) >= 4
    nd = engine.DeviceBuffer.from_numpy(nan)
    out = engine.DeviceBuffer(len(nan) * 8)
    try:
        with pytest.raises(engine.KspError) as ei:
            engine.edges_ani(nd.ptr.value, len(nan), dev.cd, 21, out.ptr.value)
        assert ei.value.code == engine.KSP_E_ARG
        with pytest.raises(engine.KspError) as ei:
            engine.components_edges_ani(dev.n, nd.ptr.value, len(nan), dev.cd, 21, 0.5)
        assert ei.value.code == engine.KSP_E_ARG
    finally:
        nd.free()
        out.free()


# ---- the drop-in calls -----------------------------------------------------------------------------------------------------------

def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def index(oracle_lib, tmp_path_factory):
    """d/index: the hostile index, .namesMap and .extra; d/full: the same with the reference's TSVs and the restated ANI column."""
    d = tmp_path_factory.mktemp("big_counts")
    ix = xv.hostile_index(1)
    (d / "index").mkdir()
    prefix = str(d / "index" / "ix")
    oracle_lib.write_index(prefix, ix["color_off"], ix["sources"], ix["color_w"], ix["group_ids"], ix["kmer_counts"])
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{ix['n_names']}\n" + "".join(f"{i + 1} genome_{i + 1}\n" for i in range(ix["n_names"])))
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    shutil.copytree(d / "index", d / "full")
    full = str(d / "full" / "ix")
    oracle_lib.ref_pairwise(full, 1)
    tsv, seq = _read(full + "_kSpider_pairwise.tsv"), _read(full + "_kSpider_seqToKmersNo.tsv")
    rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
    by_pair = {(int(r[0]), int(r[1])): r for r in rows}
    for a, b, col, target in ix["boundary"]:                               # the planted rows print what was planted
        assert by_pair[a, b][col] == xv.text(target) and xv.text(target) in ("0.2", "0.199999")
    assert all(2**24 < int(r[2]) < 2**32 for r in rows) and sum(xv.frac(xv.f32_of_int(int(r[2]))) != int(r[2]) for r in rows) > len(rows) // 2
    return SimpleNamespace(dir=d, full=full, tsv=tsv, seq=seq, rows=rows, n=ix["n_names"], ani=ani_restate.estimate_ani(full, SCALE))


def _fresh(index, tmp_path, name):
    shutil.copytree(index.dir / "index", tmp_path / name)
    return str(tmp_path / name / "ix")


def _check_tsvs(index, prefix, want=None):
    assert _read(prefix + "_kSpider_pairwise.tsv") == (index.tsv if want is None else want)
    assert _read(prefix + "_kSpider_seqToKmersNo.tsv") == index.seq
    assert not glob.glob(os.path.join(os.path.dirname(prefix), "*.partial"))


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_drop_in_calls(index, tmp_path, monkeypatch, devices):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    text, names = index.tsv.decode(), [f"genome_{i + 1}" for i in range(index.n)]
    prefix = _fresh(index, tmp_path, "pairwise")
    engine.pairwise(prefix, 2)
    _check_tsvs(index, prefix)
    for dist, col in DISTS.items():
        prefix = _fresh(index, tmp_path, dist)
        folder = os.path.dirname(prefix)
        texts = sorted({r[col] for r in index.rows}, key=float)
        for c in (0.2, float(texts[len(texts) // 2])):                     # the cut-off of the planted rows, and a row's own printed value
            want = cr.cut_tsv(text, col, c).encode()
            assert index.tsv.count(b"\n") > want.count(b"\n") > 1
            engine.pairwise_cut(prefix, 2, dist, c)
            _check_tsvs(index, prefix, want)
            engine.pairwise_and_cluster(prefix, 2, dist, c)
            _check_tsvs(index, prefix)
            path = ref_cluster.output_path(prefix, c)
            got = _read(path)
            os.remove(path)
            want = ref_cluster.write_clusters(index.full, dist, c)
            assert got == _read(want), (dist, c)
            os.remove(want)
        engine.pairwise_and_tree(prefix, 2, dist, False)
        _check_tsvs(index, prefix)
        assert _read(prefix + f"_kSpider_tree_{dist}.tsv").decode() == tr.tree_tsv(dist, index.n, [(int(r[0]), int(r[1]), r[col]) for r in index.rows]), dist
        for t in (0.2, 0.5):
            engine.pairwise_and_repr(prefix, 2, dist, t)
            _check_tsvs(index, prefix)
            assert _read(prefix + "_kSpider_repr_sketches.txt") == rr.repr_sketches(text, col, t), (dist, t)
            engine.pairwise_and_dereplicate(prefix, 2, dist, t)
            _check_tsvs(index, prefix)
            assert _read(prefix + f"_kSpider_dereplicated_{dist}.tsv") == dr.dereplicated_tsv(text, names, col, t, dist), (dist, t)
        assert not glob.glob(os.path.join(folder, "*.partial"))
    prefix = _fresh(index, tmp_path, "ani")
    engine.pairwise_ani(prefix, 2, SCALE)
    _check_tsvs(index, prefix)
    assert _read(prefix + "_kSpider_pairwise.ani_col.tsv") == index.ani

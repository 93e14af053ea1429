"""Top-k neighbours on the GPU against the restatement in tests/topk_restate.py: `index` and `count` compared for
exact equality, in both KSP_TOPK_SELECT modes (the hand-written select kernels and rocPRIM's segmented sort).  A hub on both
sides of each class limit and one that needs several refills, with what ksp_debug_topk_classes reports; k around the length of
a segment in every class and KSP_TOPK_MAX_K on a streamed one; more than k entries sharing the best value; NaN and +inf rows,
records without shared k-mers, self pairs, ends out of range, every column, three orders of the same records; the sizes where
a ballot and a chunk begin and end and a grid so small that every workgroup loops; a seeded hostile multigraph of 20 000
nodes; ranked host edges; the file-writing calls on a 400-source index, on one and on two workers, and on colours of weight 0;
the executable and the refusals.  Every output array has sentinels behind it and d_edges is compared after every call.  The
inputs come from tests/topk_inputs.py, whose properties tests/test_topk_cpu.py checks without a GPU."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import derep_inputs as di
import repr_restate as rr
import topk_inputs as ti
import topk_restate as tr
import zero_weight_inputs as zw
from kspider_amd import engine
from topk_device import FILL, MODES, NO_CLASSES, TAIL, _check, _device, _expected_classes, _same

pytestmark = pytest.mark.gpu

C = engine.TOPK_CHUNK_EDGES
W = engine.TOPK_WAVE_ENTRIES
L = engine.TOPK_LDS_ENTRIES
MAX_K = engine.TOPK_MAX_K
NONE = tr.NONE
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "topk")

# ---- 1. class limits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ti.CLASS_LIMIT_HUBS)
def test_a_hub_on_both_sides_of_every_class_limit(monkeypatch, size):
    e, cnt, n_nodes, (hub,) = ti.hubs([size])
    k = 10
    for col in (3, 4, 5):
        want, classes = _check(monkeypatch, n_nodes, e, cnt, col, k)
        assert want[1][hub] == k
        hub_class = ti.class_of(size)                                      # the definition's: by the number of entries alone
        assert classes["workgroup"] == (hub_class == "workgroup") and classes["stream"] == (hub_class == "stream"), classes
        assert classes["wave"] == int((tr.entries(e, n_nodes) > 0).sum()) - (hub_class != "wave") > 250, classes
        if hub_class == "stream":
            assert classes["refills"] == -(-size // (L - k))
    if size == 3 * L + 5:
        assert classes["refills"] == 4 > 1
    if size == L + 1:
        assert classes["refills"] == 2


# ---- 2. k against the segment ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sorted({k for n in ti.SEGMENTS for k in ti.ks_around(n)}))
def test_k_around_the_length_of_a_segment_in_every_class(monkeypatch, k):
    """A wave node of 37, a workgroup node of 200 and a streamed node of KSP_TOPK_LDS_ENTRIES + 100 entries in one graph, at
    k = 1, n - 1, n, n + 1 of the first two and at 1 and KSP_TOPK_MAX_K (a streamed segment is longer than every k)."""
    e, cnt, n_nodes, nodes = ti.hubs(ti.SEGMENTS)
    want, classes = _check(monkeypatch, n_nodes, e, cnt, 5, k)
    assert want[1][nodes].tolist() == [min(k, n) for n in ti.SEGMENTS]
    assert classes["stream"] == 1 and classes["workgroup"] == 1 and classes["refills"] == -(-ti.SEGMENTS[2] // (L - k))
    if k == MAX_K:
        assert classes["refills"] == 2


# ---- 3. ties and specials --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", ti.TIES)
def test_more_than_k_entries_share_the_best_value(monkeypatch, n, k):
    e, cnt, n_nodes, hub, best = ti.ties(n, k)
    for col in (3, 4, 5):
        want, _ = _check(monkeypatch, n_nodes, e, cnt, col, k)
        assert want[0][hub].tolist() == best[:k].tolist()                  # the lowest indices win


@pytest.mark.parametrize("col", [3, 4, 5])
def test_specials_in_three_orders(monkeypatch, col):
    """NaN and +inf rows, records with shared = 0, self pairs, ends >= n_nodes, repeated pairs in both orientations: the same
    records ascending, reversed and shuffled.  Each order against the restatement over that order; and from order to order
    every node keeps its column of values, while the records named follow the indices."""
    e, cnt, _ = ti.specials()
    n_nodes, k = len(cnt), 40                      # (more than most nodes have entries: the NaN rows at their ends are listed)
    values, records = [], []
    for name, eo in ti.orders(e).items():
        want, _ = _check(monkeypatch, n_nodes, eo, cnt, col, k)
        index, count = want
        inside = (eo["source_1"] < n_nodes) & (eo["source_2"] < n_nodes)
        v = np.full(len(eo), np.nan, dtype=np.float32)
        v[inside] = rr.column_values(eo[inside], cnt, col)
        hit = index != NONE
        values.append(np.where(hit, v[np.where(hit, index, 0)], np.float32(-1)))
        records.append(index)
        assert np.isnan(values[-1]).any() and np.isinf(values[-1]).any() and (values[-1] == 0).any(), name
    for other in values[1:]:
        assert np.array_equal(values[0], other, equal_nan=True)
    assert (records[0] != records[1]).any() and (records[0] != records[2]).any()


# ---- 4. chunks and grids ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ti.CHUNK_SIZES)
def test_ballot_and_chunk_boundaries(monkeypatch, n):
    if n == 3 * C - 7:
        monkeypatch.setenv("KSP_TOPK_MAX_WORKGROUPS", "2")                 # 3 chunks on 2 workgroups: every workgroup loops
    e, cnt = ti.random_case(n, 40)
    for col in (3, 4, 5):
        _check(monkeypatch, ti.N_RANDOM, e, cnt, col, 3)


def test_hostile_multigraph_of_20000_nodes(monkeypatch):
    e, cnt, _ = di.hostile(11, 20000, 2 * C + 1)
    for col in (3, 4, 5):
        _check(monkeypatch, 20000, e, cnt, col, 4)
    monkeypatch.setenv("KSP_TOPK_MAX_WORKGROUPS", "2")
    _check(monkeypatch, 20000, di.permuted(e, 3)[0], cnt, 4, MAX_K)


# ---- 5. ranked host edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 7, 100])
def test_ranked_host_edges_with_equal_ranks(monkeypatch, k):
    n_nodes, a, b, rank, _ = ti.ranked_case()
    want = tr.ranked(n_nodes, a, b, rank, k)
    for mode in MODES:
        monkeypatch.setenv("KSP_TOPK_SELECT", mode)
        _same(engine.topk_ranked(n_nodes, a, b, rank, k, tail=TAIL, fill=FILL), want, (mode, k))
        classes = engine.topk_classes()
        assert classes == (_expected_classes(tr.select(n_nodes, a, b, rank, 1)[2], k) if mode == "kernels" else NO_CLASSES)


# ---- 6. the files ----------------------------------------------------------------------------------------------------------------

DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The 400-source index of tests/test_repr_gpu.py with a .namesMap, the TSVs of engine.pairwise and its ANI column."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("topk")
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    (d / "index").mkdir()
    index = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(index, sk.keys, sk.offsets)
    names = [f"genome_{i + 1}" for i in range(sk.n_sources)]
    with open(index + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {name}\n" for i, name in enumerate(names)))
    shutil.copytree(d / "index", d / "full")
    prefix = str(d / "full" / "ix")
    engine.pairwise(prefix, 2)
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    engine.estimate_ani(prefix, 2, 1000)
    return dict(dir=d, prefix=prefix, tsv=_read(prefix + "_kSpider_pairwise.tsv"), seq=_read(prefix + "_kSpider_seqToKmersNo.tsv"), names=names,
                ani=_read(prefix + "_kSpider_pairwise.ani_col.tsv").decode().split("\n")[1:-1], sizes=sk.sizes.astype(np.uint32), n=sk.n_sources)


def _same_value_columns(from_tsv: bytes, from_hbm: bytes, tsv_text: str, names: list, col: int):
    """What the header promises between the two file paths: per source the value texts are equal line by line, and a row whose
    neighbour differs carries a text that occurs more than once among that source's rows of the TSV."""
    a, b = tr.per_source(from_tsv), tr.per_source(from_hbm)
    assert a.keys() == b.keys()
    texts_of = {}
    for r in tr.tsv_rows(tsv_text):
        for end in (0, 1):
            texts_of.setdefault(names[int(r[end]) - 1], []).append(r[col])
    differing = 0
    for s in a:
        assert [t for _, t in a[s]] == [t for _, t in b[s]], s
        for (na, t), (nb, _) in zip(a[s], b[s]):
            if na != nb:
                differing += 1
                assert texts_of[s].count(t) > 1, (s, t)
    return differing


@pytest.mark.parametrize("k", [1, 5])
def test_topk_over_the_tsv(full, k):
    tsv = full["tsv"].decode()
    for dist, col in DISTS.items():
        want = tr.topk_tsv(tsv, full["names"], col, k, dist)
        assert want.count(b"\n") > full["n"] // 2
        engine.topk(full["prefix"], dist, k)
        out = full["prefix"] + f"_kSpider_topk_{dist}.tsv"
        assert _read(out) == want, (dist, k)
        os.remove(out)
    want = tr.topk_tsv(tsv, full["names"], 0, k, "ani", texts=full["ani"])
    out = str(full["dir"] / f"ani_{k}.tsv")
    engine.topk(full["prefix"], "ani", k, out)
    assert _read(out) == want and len(want) > 100
    assert not glob.glob(str(full["dir"] / "full" / "*.partial")) and not glob.glob(str(full["dir"] / "full" / "*_topk_*"))


@pytest.mark.parametrize("devices,k", [(None, 1), (None, 5), ("0,0", 5)])
def test_files_from_hbm(full, monkeypatch, devices, k):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    tsv = full["tsv"].decode()
    for dist, col in DISTS.items():
        d = full["dir"] / f"fused_{dist}_{devices}_{k}"
        shutil.copytree(full["dir"] / "index", d)
        fused = str(d / "ix")
        engine.pairwise_and_topk(fused, 2, None if dist == "max_cont" else dist, k)
        assert _read(fused + "_kSpider_pairwise.tsv") == full["tsv"] and _read(fused + "_kSpider_seqToKmersNo.tsv") == full["seq"], (dist, devices)
        out = fused + f"_kSpider_topk_{dist}.tsv"
        from_hbm = _read(out)
        assert from_hbm == tr.topk_tsv_floats(tsv, full["names"], full["sizes"], col, k, dist), (dist, devices, k)
        os.remove(out)
        engine.topk(fused, dist, k)
        _same_value_columns(_read(out), from_hbm, tsv, full["names"], col)
        assert not glob.glob(str(d / "*.partial"))


@pytest.mark.parametrize("sub", ["plain", "nan"])
def test_zero_weight_colours(oracle_lib, tmp_path, sub):
    """The row 3 - 4 exists only with shared_kmers = 0 (value 0; "nan": NaN, source 4 counts 0 k-mers): merged in on the host."""
    prefix = str(tmp_path / "z")
    zw.write(oracle_lib, prefix, sub)
    names = [f"genome_{i + 1}" for i in range(6)]
    engine.pairwise(prefix, 1)
    tsv = _read(prefix + "_kSpider_pairwise.tsv")
    assert any(r[:3] == ["3", "4", "0"] for r in tr.tsv_rows(tsv.decode()))
    os.remove(prefix + "_kSpider_pairwise.tsv")
    for dist, col in DISTS.items():
        engine.pairwise_and_topk(prefix, 1, dist, 2)
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
        out = prefix + f"_kSpider_topk_{dist}.tsv"
        from_hbm = _read(out)
        assert from_hbm == tr.topk_tsv_floats(tsv.decode(), names, zw.COUNTS[sub], col, 2, dist), (sub, dist)
        hits = tr.per_source(from_hbm)
        assert [n for n, _ in hits["genome_3"]] == ["genome_4"] and [n for n, _ in hits["genome_4"]] == ["genome_3"] and len(hits) == 6
        os.remove(out)
        engine.topk(prefix, dist, 2)
        assert _read(out) == from_hbm                                       # (no two rows of a source here: nothing to choose)


# ---- 7. the executable and the refusals ------------------------------------------------------------------------------------------

def test_exe_and_refusals(full, monkeypatch):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    out = str(d / "mine.tsv")
    run = subprocess.run([EXE, prefix, "avg_cont", "3", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    engine.topk(prefix, "avg_cont", 3)
    assert _read(out) == _read(prefix + "_kSpider_topk_avg_cont.tsv") == tr.topk_tsv(full["tsv"].decode(), full["names"], 4, 3, "avg_cont")
    os.remove(out)
    os.remove(prefix + "_kSpider_topk_avg_cont.tsv")
    before = sorted(os.listdir(d))
    for call in (lambda: engine.topk(prefix, "max_cont", 0), lambda: engine.pairwise_and_topk(prefix, 1, "max_cont", 0),
                 lambda: engine.topk(prefix, "max_cont", MAX_K + 1), lambda: engine.pairwise_and_topk(prefix, 1, "max_cont", MAX_K + 1),
                 lambda: engine.topk(prefix, "jaccard", 3), lambda: engine.pairwise_and_topk(prefix, 1, "jaccard", 3),
                 lambda: engine.pairwise_and_topk(prefix, 1, "ani", 3),
                 lambda: engine.edges_topk(4, 0, 5, 0, 5, 2), lambda: engine.edges_topk(4, 0, 0, 0, 6, 2), lambda: engine.edges_topk(4, 0, 0, 0, 5, 0),
                 lambda: engine.edges_topk(4, 0, 0, 0, 5, MAX_K + 1), lambda: engine.topk_ranked(3, [0, 1], [1, 3], [1, 1], 2)):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    for args, code in ((["ani2", "3"], 1), (["max_cont", "0"], 1), (["max_cont", "x"], 2), (["max_cont"], 2)):
        run = subprocess.run([EXE, prefix] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert run.returncode == code and run.stderr, args
    assert sorted(os.listdir(d)) == before
    # a bad device: KSP_E_HIP with the entry's name
    with pytest.raises(engine.KspError) as ei:
        engine.edges_topk(4, 0, 0, 0, 5, 2, device=99)
    assert ei.value.code == engine.KSP_E_HIP and "ksp_edges_topk: no such device" in str(ei.value)
    monkeypatch.setenv("KSPIDER_DEVICE", "99")
    with pytest.raises(engine.KspError) as ei:
        engine.topk(prefix, "max_cont", 3)
    assert ei.value.code == engine.KSP_E_HIP and "ksp_topk_ranked: no such device" in str(ei.value) and sorted(os.listdir(d)) == before
    monkeypatch.delenv("KSPIDER_DEVICE")
    # no record at all: all counts 0, all slots 0xFFFFFFFF, no kernel runs
    for mode in MODES:
        monkeypatch.setenv("KSP_TOPK_SELECT", mode)
        index, count = engine.edges_topk(5, 0, 0, 0, 5, 3, tail=TAIL, fill=FILL)
        assert (index == NONE).all() and index.shape == (5, 3) and (count == 0).all() and engine.topk_classes() == NO_CLASSES
    monkeypatch.setenv("KSP_TOPK_SELECT", "quicksort")
    with pytest.raises(engine.KspError) as ei:
        _device(3, di.edges([0], [1]), di.same(3), 5, 1)
    assert ei.value.code == engine.KSP_E_ARG and "KSP_TOPK_SELECT" in str(ei.value)
    monkeypatch.delenv("KSP_TOPK_SELECT")
    # a malformed row: refused before any file is written
    with open(prefix + "_kSpider_pairwise.tsv", "ab") as f:
        f.write(b"1\t2\t5\tzero\tzero\tzero\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.topk(prefix, "max_cont", 3)
    assert ei.value.code == engine.KSP_E_IO and "malformed" in str(ei.value) and sorted(os.listdir(d)) == before
    with open(prefix + "_kSpider_pairwise.tsv", "wb") as f:
        f.write(full["tsv"])
    # an id missing from .namesMap: the TSV path refuses the row that names it, the fused call the source
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.topk(prefix, "max_cont", 3)
    assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value) and sorted(os.listdir(d)) == before
    os.remove(prefix + "_kSpider_pairwise.tsv")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise_and_topk(prefix, 1, "max_cont", 3)
    assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value) and sorted(os.listdir(d)) == before

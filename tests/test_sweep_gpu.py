"""The cut-off ladder on the GPU against the restatement in tests/sweep_restate.py: the level byte of every
record and the bands the scatter fills (ksp_debug_sweep_bands) at the sizes where a ballot (64 records) and a chunk
(SWEEP_CHUNK_EDGES records) begin and end and with a grid so small that every workgroup loops; the components continued from
band to band (ksp_components_sweep) against a union-find per rank; the join's own records (ksp_components_edges_sweep) and the
two file-writing calls against oracle.ref_cluster, cut-off by cut-off.

A cut-off of mode 1 (ksp::cc_critical: not even +inf passes) cannot be asked for through the ABI: the text "inf" times 100 is
below no threshold, and a NaN cut-off is refused.  What stands in for it here are the cut-offs 2.0 and +inf, which no
containment — for +inf no finite value — passes, so that the top ranks are passed by NaN records only."""
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cut_restate as cr
import sweep_restate as sr
from kspider_amd import engine
from oracle import ref_cluster

pytestmark = pytest.mark.gpu

C = engine.SWEEP_CHUNK_EDGES
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "clusters")
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "cluster_sweep")
TAIL = 7                        # sentinel entries behind the last one an output array could hold
N_NODES = 5200
COUNT = 25600                   # k-mers of every source of the pattern cases: shared / COUNT is the value of all three columns


def _edges(s1, s2, shared):
    e = np.zeros(len(s1), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = s1, s2, shared
    return e


def _device_bands(edges, kmer_counts, col, cutoffs):
    """(level[n], off[K + 1], a, b) of ksp_debug_sweep_bands; asserts the sentinels behind every output and the input intact."""
    n = len(edges)
    ed = engine.DeviceBuffer.from_numpy(edges) if n else None
    cd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(kmer_counts, dtype=np.uint32))
    ld = engine.DeviceBuffer.from_numpy(np.full(n + TAIL, 0xA5, dtype=np.uint8))
    ad = engine.DeviceBuffer.from_numpy(np.full(n + TAIL, 0xDEADBEEF, dtype=np.uint32))
    bd = engine.DeviceBuffer.from_numpy(np.full(n + TAIL, 0xFEEDFACE, dtype=np.uint32))
    try:
        off = engine.sweep_bands(ed.ptr.value if ed else 0, n, cd.ptr.value, col, cutoffs, ld.ptr.value, ad.ptr.value, bd.ptr.value)
        level, a, b = ld.to_numpy(np.uint8, n + TAIL), ad.to_numpy(np.uint32, n + TAIL), bd.to_numpy(np.uint32, n + TAIL)
        kept = int(off[-1])
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and kept <= n
        assert (level[n:] == 0xA5).all(), "a level byte behind the last record was written"
        assert (a[kept:] == 0xDEADBEEF).all() and (b[kept:] == 0xFEEDFACE).all(), "an endpoint behind the last band was written"
        if n:
            assert (ed.to_numpy(engine.EDGE_DTYPE, n) == edges).all(), "d_edges was written"
        return level[:n], off, a[:kept], b[:kept]
    finally:
        for buf in (ed, cd, ld, ad, bd):
            if buf:
                buf.free()


def _check_bands(edges, want_level, K, got, what):
    level, off, a, b = got
    assert (level == want_level).all(), what
    assert (np.diff(off.astype(np.int64)) == np.bincount(want_level, minlength=K + 1)[1:]).all(), what
    band = np.repeat(np.arange(1, K + 1), np.diff(off.astype(np.int64)))
    have = np.sort(np.rec.fromarrays([band, a, b], names="l,a,b"), order=["l", "a", "b"])
    m = want_level > 0
    want = np.sort(np.rec.fromarrays([want_level[m].astype(np.int64), edges["source_1"][m], edges["source_2"][m]], names="l,a,b"), order=["l", "a", "b"])
    assert len(have) == len(want) and (have == want).all(), what


def _ladder(K):
    """K cut-offs j * step / 256 and the value of level L between the L-th and the next: (L * step + step / 2) / 256."""
    step = 256 // (K + 1)
    return step, [j * step / 256 for j in range(1, K + 1)]


def _pattern_edges(level_of, step):
    i = np.arange(len(level_of))
    return _edges(i // 4000, 1000 + i % 4000, (level_of.astype(np.int64) * step * 100 + step * 50) * (COUNT // 25600))


def _patterns(n, K):
    i = np.arange(n)
    edge = np.where(i < C, K, 1) if n > C else np.where(i == n - 1, 1, K)      # the level changes exactly at a chunk's edge (at the last record when shorter)
    return {"one_level": np.full(n, K), "level_0": np.zeros(n, dtype=np.int64), "lane_by_lane": i % (K + 1), "chunk_edge": edge}


@pytest.mark.parametrize("K", [1, 2, 7, 255])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17])
def test_levels_and_bands_at_ballot_and_chunk_boundaries(n, K):
    cnt = np.full(N_NODES, COUNT, dtype=np.uint32)
    step, cutoffs = _ladder(K)
    shuffled = list(np.random.default_rng(K).permutation(cutoffs))             # the caller's order does not matter to a level
    for name, level_of in _patterns(n, K).items():
        e = _pattern_edges(level_of, step)
        want = sr.levels(sr.column_texts(e, cnt, 5), shuffled)
        assert (want == level_of).all()                                        # (the restatement agrees with how the case was built)
        for col in (3, 4, 5):
            _check_bands(e, want, K, _device_bands(e, cnt, col, shuffled), (n, K, name, col))


def _random_case(n, K, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(3000, 4001, size=N_NODES).astype(np.uint32)
    i = np.arange(n)
    s1, s2 = i // 4000, 1000 + i % 4000
    u = rng.uniform(0.02, 0.4, size=n)
    shared = np.floor(u * 2.0 / (1.0 / cnt[s1] + 1.0 / cnt[s2])).astype(np.uint64)
    e = _edges(s1, s2, shared)[rng.permutation(n)]
    cutoffs = list(rng.permutation(np.linspace(0.05, 0.35, K)))
    return e, cnt, cutoffs


def test_every_workgroup_loops_over_chunks(monkeypatch):
    """40 chunks (the last one short) on a grid of 3 workgroups: 13 or 14 chunks each, 7 cut-offs in every column."""
    monkeypatch.setenv("KSP_SWEEP_MAX_WORKGROUPS", "3")
    e, cnt, cutoffs = _random_case(40 * C - 5, 7, 40)
    for col in (3, 4, 5):
        want = sr.levels(sr.column_texts(e, cnt, col), cutoffs)
        assert len(np.unique(want)) == 8
        _check_bands(e, want, 7, _device_bands(e, cnt, col, cutoffs), col)


def _float(bits: int) -> np.float32:
    return np.float32(struct.unpack("<f", struct.pack("<I", bits))[0])


def _critical(cutoff):
    """The smallest non-negative float whose text is kept, by bisection over the bit patterns with the restatement as the test."""
    lo, hi = 0, 0x7F800000
    assert cr.keep(engine.format_float(_float(hi)), cutoff) and not cr.keep(engine.format_float(_float(lo)), cutoff)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cr.keep(engine.format_float(_float(mid)), cutoff):
            hi = mid
        else:
            lo = mid
    return hi


@pytest.mark.parametrize("cutoff", [0.8, 0.6, 0.95])
def test_critical_floats_nan_and_cutoffs_nothing_passes(cutoff):
    """Sources of 2^24 k-mers: shared / 2^24 is exact for every float in [0.5, 1), so the critical float of a cut-off and its two
    neighbours are the values of three records; two NaN records (no k-mers, nothing shared); cut-offs below 0 (everything
    passes), 2.0 and +inf (only NaN passes) and the cut-off twice."""
    crit = _critical(cutoff)
    vals = [_float(crit - 1), _float(crit), _float(crit + 1)]
    assert vals[1] < np.float32(cutoff)
    shared = [int(float(v) * 2.0**24) for v in vals]
    cnt = np.array([2**24, 2**24, 0, 0, 0, 9], dtype=np.uint32)             # (the last record: 3 shared of 0 and 9 k-mers, an infinite containment)
    e = _edges([0, 0, 0, 2, 2, 4], [1, 1, 1, 3, 4, 5], shared + [0, 0, 3])
    cutoffs = [2.0, cutoff, -0.5, float("inf"), cutoff]
    for col in (3, 4, 5):
        texts = sr.column_texts(e, cnt, col)
        assert texts[:3] == [engine.format_float(float(v)) for v in vals] and "nan" in texts[3] and "nan" in texts[4]
        want = sr.levels(texts, cutoffs)
        assert want[:5].tolist() == [1, 3, 3, 5, 5], (col, want)        # below the critical float: only the cut-off below 0; NaN: all five
        _check_bands(e, want, 5, _device_bands(e, cnt, col, cutoffs), (col, cutoff))
        ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
        try:
            labels, kept = engine.components_edges_sweep(6, ed.ptr.value, len(e), cd.ptr.value, col, cutoffs)
        finally:
            ed.free(); cd.free()
        want_labels, want_kept = sr.ladder(6, e, texts, cutoffs)
        assert (labels == want_labels).all() and (kept == want_kept).all(), (col, cutoff)


# ---- continued components ------------------------------------------------------------------------------------------------

def _sweep_case(n, a, b, level, K):
    a, b, level = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32), np.asarray(level, dtype=np.uint8)
    got = engine.components_sweep(n, a, b, level, K)
    want = sr.per_rank_components(n, a, b, level, K)
    assert got.shape == want.shape and (got == want).all()
    return got


def test_continued_components_chain_stars_duplicates_and_empty_bands():
    rng = np.random.default_rng(3)
    # a 4 096-node chain in reversed, shuffled order, levels alternating 1 / 2: rank 1 has pairs, rank 0 the whole chain
    n = 4096
    a, b = np.arange(n - 1, 0, -1), np.arange(n - 2, -1, -1)
    p = rng.permutation(n - 1)
    got = _sweep_case(n, a[p], b[p], (1 + a % 2)[p], 2)
    assert (got[0] == 0).all() and len(np.unique(got[1])) == n // 2
    # two stars joined only at level 1; K = 3 with an empty band 2
    hub1, hub2 = 500, 20
    a = np.concatenate([np.full(300, hub1), np.full(300, hub2), [1001]])
    b = np.concatenate([np.arange(1000, 1300), np.arange(2000, 2300), [2001]])
    got = _sweep_case(2400, a, b, np.concatenate([np.full(600, 3), [1]]), 3)
    assert got[2][1000] == hub1 and got[1][2299] == hub2 and (got[1] == got[2]).all() and got[0][hub1] == hub2
    # an edge at level 1 that duplicates a level-3 connection; self loops; isolated nodes
    _sweep_case(10, [1, 2, 1, 5, 7, 7], [2, 3, 3, 5, 7, 8], [3, 3, 1, 2, 1, 2], 3)
    # empty middle bands: levels 1 and 6 only, K = 6
    a = rng.integers(0, 3000, size=2500)
    b = rng.integers(0, 3000, size=2500)
    _sweep_case(3000, a, b, rng.choice([0, 1, 6], size=2500), 6)
    # every band filled, more than one chunk, random graph
    a = rng.integers(0, 20000, size=3 * C + 17)
    b = rng.integers(0, 20000, size=3 * C + 17)
    _sweep_case(20000, a, b, rng.integers(0, 8, size=3 * C + 17), 7)


def test_continued_components_hooked_root_chains():
    """Roots hooked into a chain of five in ONE pass over a band (40 -> 30 -> 20 -> 10 -> 5), while an edge of the same band
    reaches a smaller label (2) through a leaf of the deepest star.  A round of hook + two jumps leaves node 10, a non-root,
    as the label of node 41; hooking again at that point would move 10 under 2 and leave its former leaves 11 and 12, which
    have jumped to 5, behind — the components of the rank above are only safe when every hook pass starts from stars."""
    a = [10, 10, 40, 11, 20, 30, 40, 41, 50]
    b = [11, 12, 41, 5, 12, 20, 30, 50, 2]
    level = [2, 2, 2, 1, 1, 1, 1, 1, 1]
    got = _sweep_case(51, a, b, level, 2)
    assert set(got[0][[2, 5, 10, 11, 12, 20, 30, 40, 41, 50]].tolist()) == {2}
    # the same with every star 200 leaves wide and the chain 60 roots long
    rng = np.random.default_rng(8)
    roots = np.arange(100, 100 + 60 * 300, 300)
    a2 = np.concatenate([np.repeat(roots, 200), roots[1:] + 1, [roots[-1] + 2, 19000]])
    b2 = np.concatenate([(roots[:, None] + 1 + np.arange(200)[None, :]).ravel(), roots[:-1] + 2, [19000, 3]])
    lv = np.concatenate([np.full(60 * 200, 2), np.full(59 + 2, 1)])
    p = rng.permutation(len(a2))
    _sweep_case(19001, a2[p], b2[p], lv[p], 2)


def test_continued_components_limits_and_refusals():
    assert engine.components_sweep(1, [], [], [], 4).tolist() == [[0]] * 4               # one node, no edge
    assert (engine.components_sweep(7, [], [], [], 2) == np.arange(7)).all()
    assert engine.components_sweep(0, [], [], [], 3).shape == (3, 0)
    assert (engine.components_sweep(3, [0, 1], [1, 2], [0, 0], 2) == np.arange(3)).all()   # every edge in level 0
    # K = 255 with one edge per level on a 256-node path: rank r joins the nodes r .. 255 ... in the order of the path
    path = np.arange(255)
    got = _sweep_case(256, path, path + 1, np.arange(1, 256), 255)
    assert (got[0] == 0).all() and len(np.unique(got[254])) == 255
    with pytest.raises(engine.KspError) as ei:
        engine.components_sweep(5, [1], [5], [1], 2)
    assert ei.value.code == engine.KSP_E_ARG and "out of range" in str(ei.value)


# ---- the join's own records ----------------------------------------------------------------------------------------------

def test_sweep_over_device_edge_records():
    """The 3 000-source join of tests/test_cluster.py: six cut-offs in shuffled order with one duplicate, per column; labels
    and kept counts row by row, and row by row equal to what ksp_components_edges gives for that cut-off alone."""
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
        texts = sr.column_texts(ev, sk.sizes, col)
        mid = float(sorted(texts, key=float)[m // 2])                      # a printed value of the column is a cut-off
        cutoffs = [0.5, 0.0, mid, 0.1, 2.0, 0.3, mid]
        want_labels, want_kept = sr.ladder(sk.n_sources, ev, texts, cutoffs)
        assert 0 < want_kept[2] < m and want_kept[1] == m and want_kept[4] == 0
        labels, kept = engine.components_edges_sweep(sk.n_sources, ed.ptr.value, m, cnt_d.ptr.value, col, cutoffs)
        assert (kept == want_kept).all(), (col, kept, want_kept)
        for i, c in enumerate(cutoffs):
            assert (labels[i] == want_labels[i]).all(), (col, c)
        assert (labels[3] == engine.components_edges(sk.n_sources, ed.ptr.value, m, cnt_d.ptr.value, col, 0.1)).all()
    assert (ed.to_numpy(engine.EDGE_DTYPE, m) == ev).all()
    eng.close()
    for buf in (keys_d, cnt_d, ed):
        buf.free()


# ---- files ---------------------------------------------------------------------------------------------------------------

DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The 400-source index of tests/test_cluster.py, the TSV of engine.pairwise, and per distance the ladder {0, the printed
    values at 1/4, 1/2 and 3/4 of the sorted distinct ones, 1} with what the oracle writes for each of its cut-offs."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("sweep")
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    (d / "index").mkdir()
    index = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(index, sk.keys, sk.offsets)
    _names_map(index, sk.n_sources)
    shutil.copytree(d / "index", d / "full")
    prefix = str(d / "full" / "ix")
    engine.pairwise(prefix, 2)
    tsv = _read(prefix + "_kSpider_pairwise.tsv")
    rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
    ladders, want = {}, {}
    for dist, col in DISTS.items():
        distinct = sorted({r[col] for r in rows}, key=float)
        assert len(distinct) >= 4
        ladder = [0.0] + [float(distinct[len(distinct) * q // 4]) for q in (1, 2, 3)] + [1.0]
        assert len(set(ladder)) == 5
        ladders[dist] = ladder
        for c in ladder:
            path = ref_cluster.write_clusters(prefix, dist, c)
            want[dist, c] = (os.path.basename(path), _read(path))
            os.remove(path)
    return dict(dir=d, prefix=prefix, tsv=tsv, rows=rows, ladders=ladders, want=want, n=sk.n_sources)


def _check_outputs(full, prefix, dist, given):
    """Cluster files byte-equal to the oracle's, the summary rows, no .partial and no other new file."""
    col, folder = DISTS[dist], os.path.dirname(prefix)
    distinct = sorted(set(given))
    names = set()
    summary = ["cutoff_percent\tedges\tclusters\tsingletons\tlargest"]
    for c in distinct:
        name, data = full["want"][dist, c]
        names.add(name)
        assert _read(os.path.join(folder, name)) == data, (dist, c)
        sizes = [l.count(b",") + 1 for l in data.split(b"\n") if l]
        edges = sum(cr.keep(r[col], c) for r in full["rows"])
        summary.append(f"{float(c) * 100}\t{edges}\t{len(sizes)}\t{sizes.count(1)}\t{max(sizes)}")
    assert _read(prefix + f"_kSpider_cluster_sweep_{dist}.tsv").decode() == "\n".join(summary) + "\n"
    assert {os.path.basename(p) for p in glob.glob(prefix + "_kSpider_clusters_*")} == names
    assert not glob.glob(os.path.join(folder, "*.partial"))
    assert int(summary[1].split("\t")[1]) == len(full["rows"])                                      # (cut-off 0 keeps every row)
    middle = [int(s.split("\t")[1]) for s in summary[1:]]
    assert middle == sorted(middle, reverse=True) and len(set(middle[:4])) == 4                     # the three middle bands are not empty


@pytest.mark.parametrize("dist", list(DISTS))
def test_cluster_sweep_files(full, dist):
    d = full["dir"] / f"files_{dist}"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    ladder = full["ladders"][dist]
    given = [ladder[3], ladder[0], ladder[4], ladder[1], ladder[3], ladder[2]]       # shuffled, one cut-off twice
    engine.cluster_sweep(prefix, dist, given)
    _check_outputs(full, prefix, dist, given)
    for path in glob.glob(prefix + "_kSpider_cluster*"):
        os.remove(path)
    engine.cluster_sweep(prefix, dist, [ladder[2]])                                   # a ladder of one
    name, data = full["want"][dist, ladder[2]]
    assert _read(os.path.join(str(d), name)) == data


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_pairwise_and_cluster_sweep_files(full, monkeypatch, devices):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    for dist in DISTS:
        d = full["dir"] / f"fused_{dist}_{devices}"
        shutil.copytree(full["dir"] / "index", d)
        prefix = str(d / "ix")
        ladder = full["ladders"][dist]
        given = [ladder[2], ladder[4], ladder[0], ladder[2], ladder[3], ladder[1]]
        engine.pairwise_and_cluster_sweep(prefix, 2, dist, given)
        assert _read(prefix + "_kSpider_pairwise.tsv") == full["tsv"], (dist, devices)
        _check_outputs(full, prefix, dist, given)


def test_exe_and_refusals_leave_no_file(full):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    before = sorted(os.listdir(d))
    for call in (lambda: engine.cluster_sweep(prefix, "jaccard", [0.5]), lambda: engine.cluster_sweep(prefix, "max_cont", []),
                 lambda: engine.cluster_sweep(prefix, "max_cont", [0.1] * 256), lambda: engine.cluster_sweep(prefix, "max_cont", [0.1, float("nan")]),
                 lambda: engine.pairwise_and_cluster_sweep(prefix, 1, "ani", [0.5]), lambda: engine.pairwise_and_cluster_sweep(prefix, 1, "max_cont", [])):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_sweep(prefix, "ani", [0.5])                     # ANI without its column file, as kspider_cluster refuses it
    assert "ani_col" in str(ei.value)
    assert sorted(os.listdir(d)) == before
    ladder = full["ladders"]["max_cont"]
    run = subprocess.run([EXE, prefix, "max_cont"] + [repr(c) for c in ladder], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    _check_outputs(full, prefix, "max_cont", ladder)
    run = subprocess.run([EXE, prefix, "jaccard", "0.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"jaccard" in run.stderr
    # a namesMap that does not cover the nodes: refused like kspider_cluster, and nothing new is left behind
    for path in glob.glob(prefix + "_kSpider_cluster*"):
        os.remove(path)
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_sweep(prefix, "max_cont", ladder)
    assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(d)) == before


def _as_sets(path):
    return sorted(tuple(sorted(l.rstrip("\n").split(","))) for l in open(path) if l.strip())


@pytest.mark.parametrize("tag", ["setA", "setB"])
def test_golden_ladders(tag, tmp_path):
    shutil.copytree(os.path.join(GOLD, tag), tmp_path / tag)
    prefix = str(tmp_path / tag / "sigs")
    for dist, cutoffs in (("max_cont", [1.0, 0.0, 0.3]), ("min_cont", [0.5, 0.07]), ("avg_cont", [0.25])):
        engine.cluster_sweep(prefix, dist, cutoffs)
        for c in cutoffs:
            path = ref_cluster.output_path(prefix, c)                  # (0.07 -> ..._7.000000000000001%.tsv, as the reference names it)
            assert _as_sets(path) == _as_sets(os.path.join(GOLD, tag, f"ref_{dist}_{c}.clusters")), (tag, dist, c)
            got = _read(path)
            os.remove(path)
            assert got == _read(ref_cluster.write_clusters(prefix, dist, c))
            os.remove(path)


def test_ani_on_the_file_path(full):
    d = full["dir"] / "ani"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    engine.estimate_ani(prefix, 2, 1000)
    vals = sorted({float(v) for v in _read(prefix + "_kSpider_pairwise.ani_col.tsv").decode().split("\n")[1:-1]})
    assert len(vals) >= 4
    cutoffs = [vals[len(vals) // 2], 0.0, 1.0, vals[len(vals) // 4], vals[3 * len(vals) // 4]]
    engine.cluster_sweep(prefix, "ani", cutoffs)
    summary = _read(prefix + "_kSpider_cluster_sweep_ani.tsv").decode().split("\n")
    assert [s.split("\t")[0] for s in summary[1:-1]] == [str(float(c) * 100) for c in sorted(cutoffs)]
    for c in cutoffs:
        path = ref_cluster.output_path(prefix, c)
        got = _read(path)
        os.remove(path)
        assert got == _read(ref_cluster.write_clusters(prefix, "ani", c)), c
        os.remove(path)


def test_zero_weight_colours(oracle_lib, tmp_path):
    """Rows that exist only with shared_kmers = 0 are classified on the host and united into every rank they pass.  Colours:
    {1, 2} weight 7; {3, 4} weight 0 (the pair shares nothing else); {5, 6} weight 0 AND {5, 6} weight 1 (an ordinary row)."""
    co = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
    src = np.array([1, 2, 3, 4, 5, 6, 5, 6], dtype=np.uint32)
    w = np.array([7, 0, 0, 1], dtype=np.uint32)
    ids = np.arange(1, 7, dtype=np.uint32)
    cutoffs = [0.5, 0.0, -1.0, 0.02, 2.0]
    for sub, counts in (("plain", [10, 20, 30, 40, 50, 60]), ("nan", [10, 20, 30, 0, 50, 60])):      # nan: the row 3-4 is a NaN row, kept everywhere
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
        engine.pairwise_and_cluster_sweep(prefix, 1, "max_cont", cutoffs)
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
        summary = _read(prefix + "_kSpider_cluster_sweep_max_cont.tsv").decode().split("\n")[1:-1]
        assert [int(s.split("\t")[1]) for s in summary] == [sum(cr.keep(r[5], c) for r in rows) for c in sorted(cutoffs)], sub
        for c in cutoffs:
            path = ref_cluster.output_path(prefix, c)
            got = _read(path)
            os.remove(path)
            assert got == _read(ref_cluster.write_clusters(prefix, "max_cont", c)), (sub, c)
            os.remove(path)

"""Representative sketches on the GPU: neighbour counts over the join's edge records and their ranking,
against the restatement of apps/repr_sketches.cpp in tests/repr_restate.py — every edge through its own '%.6g' text and
strtof, no critical float.  Counts are compared exactly, at the sizes where the counting kernel changes path
(kDegreeLdsNodes: LDS counters up to there, global atomics above; KSP_DEGREE_LDS=0 forces the latter) and on the edge
lists that stress the wave-level combining of equal nodes (stars, runs of 1 / 63 / 64 / 65, chains)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import repr_restate as rr
from kspider_amd import engine

pytestmark = pytest.mark.gpu

LDS_NODES = 16384      # kDegreeLdsNodes in repr.hip
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "repr_sketches")


def _edges(s1, s2, shared):
    e = np.zeros(len(s1), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = s1, s2, shared
    return e


def _device_degrees(edges, kmer_counts, col=4, threshold=0.20, n_nodes=None, ranked=False):
    n = len(kmer_counts) if n_nodes is None else n_nodes
    ed = engine.DeviceBuffer.from_numpy(edges) if len(edges) else None
    cd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(kmer_counts, dtype=np.uint32))
    try:
        f = engine.edges_repr if ranked else engine.edges_degrees
        return f(n, ed.ptr.value if ed else 0, len(edges), cd.ptr.value, col, threshold)
    finally:
        if ed:
            ed.free()
        cd.free()


def test_boundary_floats_of_the_text_test():
    """avg_cont at 0.20: 1/5 passes; 0.199999601 prints "0.2" and passes (a device comparing v > 0.2 fails here);
    0.1999994 prints "0.199999" and fails; a NaN (0 shared, a source of 0 k-mers) fails without an error."""
    cnt = np.array([5, 5, 10**7, 10**7, 10**7, 10**7, 0, 7], dtype=np.uint32)
    e = _edges([0, 2, 4, 6], [1, 3, 5, 7], [1, 1999996, 1999994, 0])
    vals = rr.column_values(e, cnt, 4)
    assert ["%.6g" % v for v in vals.tolist()] == ["0.2", "0.2", "0.199999", "nan"]
    assert vals[1] < np.float32(0.2)
    want = np.array([1, 1, 1, 1, 0, 0, 0, 0], dtype=np.uint32)
    assert (rr.degrees(e, cnt, 4, 0.20) == want).all()
    assert (_device_degrees(e, cnt) == want).all()
    node, count = _device_degrees(e, cnt, ranked=True)
    assert node.tolist() == [0, 1, 2, 3] and count.tolist() == [1, 1, 1, 1]


@functools.lru_cache(maxsize=None)
def _random_graph(n_nodes):
    """~5 * 10^4 edges over n_nodes nodes, values spread around 0.2 in all three columns; the first edges name nodes of
    the first and of the last 64 of the range and pass.  Returns (sorted edges, shuffled edges, k-mer counts,
    {col: brute-force degrees})."""
    rng = np.random.default_rng(n_nodes)
    m = 50_000
    cnt = rng.integers(3000, 4001, size=n_nodes).astype(np.uint32)
    a = rng.integers(0, n_nodes, size=m)
    b = rng.integers(0, n_nodes, size=m)
    b = np.where(a == b, (a + 1) % n_nodes, b)
    a[:4] = [0, 63, 7, 1]
    b[:4] = [n_nodes - 1, n_nodes - 64, n_nodes - 33, 2]
    s1, s2 = np.minimum(a, b), np.maximum(a, b)
    u = rng.uniform(0.02, 0.4, size=m)
    u[:4] = 0.3
    shared = np.floor(u * 2.0 / (1.0 / cnt[s1] + 1.0 / cnt[s2])).astype(np.uint64)
    e = _edges(s1, s2, shared)
    srt = e[np.lexsort((s2, s1))]
    shuf = e[rng.permutation(m)]
    want = {col: rr.degrees(srt, cnt, col, 0.20) for col in (3, 4, 5)}
    for col in (3, 4, 5):
        frac = int(want[col].sum()) / (2 * m)
        assert 1 / 3 < frac < 2 / 3, (col, frac)
        assert want[col][:64].any() and want[col][-64:].any() and want[col][n_nodes - 1] > 0 and want[col][0] > 0
    return srt, shuf, cnt, want


@pytest.mark.parametrize("n_nodes,lds", [(LDS_NODES - 1, True), (LDS_NODES, True), (LDS_NODES + 1, True), (LDS_NODES, False)])
def test_random_graphs_on_both_sides_of_the_lds_switch(monkeypatch, n_nodes, lds):
    srt, shuf, cnt, want = _random_graph(n_nodes)
    if not lds:
        monkeypatch.setenv("KSP_DEGREE_LDS", "0")
    for col in (3, 4, 5):
        for name, e in (("sorted", srt), ("shuffled", shuf)):
            got = _device_degrees(e, cnt, col, 0.20)
            assert (got == want[col]).all(), (n_nodes, lds, col, name, int(np.abs(got.astype(np.int64) - want[col]).sum()))


def _mixed_shared(m, cnt_value, every=7):
    """all edges pass (containment 1) except every `every`-th (containment 0.001): runs are broken by lanes that add nothing"""
    shared = np.full(m, cnt_value, dtype=np.uint64)
    shared[every - 1::every] = cnt_value // 1000
    return shared


@functools.lru_cache(maxsize=None)
def _combining_cases():
    """{name: (edges, k-mer counts, brute-force degrees)}: every list fits the LDS path and is also run on the global one."""
    out = {}
    n, m = LDS_NODES, 100_000
    cnt = np.full(n, 1000, dtype=np.uint32)
    j = np.arange(m)
    # a star: node 0 is source_1 of 10^5 edges; and one whose centre is the last node, source_2 of every edge
    out["star_first"] = _edges(np.zeros(m, np.uint32), 1 + j % (n - 1), _mixed_shared(m, 1000))
    out["star_last"] = _edges(j % (n - 1), np.full(m, n - 1, np.uint32), _mixed_shared(m, 1000))
    # sorted list whose source_1 runs are 1, 63, 64 or 65 edges long, in an order that moves the runs across the wave
    rng = np.random.default_rng(65)
    lens = rng.choice([1, 63, 64, 65], size=300)
    lens[:8] = [64, 64, 1, 63, 65, 65, 1, 64]
    s1 = np.repeat(np.arange(300), lens)
    s2 = s1 + 1 + np.concatenate([np.arange(k) for k in lens])
    out["runs"] = _edges(s1, s2, _mixed_shared(len(s1), 1000, every=11))
    out["runs_all_pass"] = _edges(s1, s2, np.full(len(s1), 1000, np.uint64))
    # a chain: source_2 of lane l is source_1 of lane l + 1
    c = np.arange(10_000)
    out["chain"] = _edges(c, c + 1, _mixed_shared(len(c), 1000, every=5))
    return {k: (e, cnt, rr.degrees(e, cnt, 4, 0.20)) for k, e in out.items()}


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["star_first", "star_last", "runs", "runs_all_pass", "chain"])
def test_stars_runs_and_chains_count_exactly(monkeypatch, name, lds):
    e, cnt, want = _combining_cases()[name]
    if not lds:
        monkeypatch.setenv("KSP_DEGREE_LDS", "0")
    if name == "star_first":
        assert want[0] == 100_000 - 100_000 // 7
    if name == "runs_all_pass":
        assert int(want.sum()) == 2 * len(e)
    got = _device_degrees(e, cnt)
    assert (got == want).all(), (name, lds, int(np.abs(got.astype(np.int64) - want).sum()))


def test_star_above_the_lds_switch():
    """10^5 distinct neighbours: 100 001 nodes, global counters without any switch."""
    m = 100_000
    cnt = np.full(m + 1, 1000, dtype=np.uint32)
    e = _edges(np.zeros(m, np.uint32), 1 + np.arange(m), _mixed_shared(m, 1000))
    want = rr.degrees(e, cnt, 4, 0.20)
    assert want[0] == m - m // 7
    assert (_device_degrees(e, cnt) == want).all()


def test_ranking_order_and_empty_results():
    rng = np.random.default_rng(7)
    n, m = 1000, 3000
    cnt = rng.integers(3000, 4001, size=n).astype(np.uint32)
    a = rng.integers(0, 900, size=m)                 # nodes 900.. have no edge at all
    b = rng.integers(0, 900, size=m)
    b = np.where(a == b, (a + 1) % 900, b)
    s1, s2 = np.minimum(a, b), np.maximum(a, b)
    shared = np.floor(rng.uniform(0.02, 0.4, size=m) * 3000).astype(np.uint64)
    e = _edges(s1, s2, shared)
    want = rr.degrees(e, cnt, 4, 0.20)
    rank = rr.ranked({v: int(c) for v, c in enumerate(want)})
    assert len(rank) < 900 and len(set(c for _, c in rank)) < 20        # zero-count nodes exist, and many equal counts
    node, count = _device_degrees(e, cnt, ranked=True)
    assert list(zip(node.tolist(), count.tolist())) == rank
    assert len(node) == int((want > 0).sum())
    # no edge at all, and no edge that passes: nothing ranked, all-zero degrees
    empty = e[:0]
    assert (_device_degrees(empty, cnt) == 0).all() and len(_device_degrees(empty, cnt)) == n
    assert len(_device_degrees(empty, cnt, ranked=True)[0]) == 0
    for thr in (2.0, float("inf")):
        assert (_device_degrees(e, cnt, threshold=thr) == 0).all()
        assert len(_device_degrees(e, cnt, threshold=thr, ranked=True)[0]) == 0
    # every finite value passes a negative threshold
    assert int(_device_degrees(e, cnt, threshold=-1.0).sum()) == 2 * m
    with pytest.raises(engine.KspError) as ei:
        engine.edges_degrees(n, 0, 5, 0)
    assert ei.value.code == engine.KSP_E_ARG


def _index(oracle_lib, tmp_path):
    from kspider_amd import synth
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    d = tmp_path / "a"
    d.mkdir()
    prefix = str(d / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    return prefix


def test_files_two_steps_one_pass_exe_and_failures(oracle_lib, tmp_path, monkeypatch):
    prefix = _index(oracle_lib, tmp_path)
    other = tmp_path / "b"
    shutil.copytree(tmp_path / "a", other)
    engine.pairwise(prefix, 2)
    tsv_path = prefix + "_kSpider_pairwise.tsv"
    tsv = open(tsv_path, "rb").read()
    seq = open(prefix + "_kSpider_seqToKmersNo.tsv", "rb").read()
    rows = tsv.decode().split("\n")[1:-1]
    passing = sum(rr.text_passes(r.split("\t")[4]) for r in rows)
    assert 0.05 * len(rows) <= passing <= 0.95 * len(rows), (passing, len(rows))
    # two steps: the tool over the TSV
    out = str(tmp_path / "ranking.txt")
    engine.repr_sketches(tsv_path, None, 0.20, out)
    want = rr.repr_sketches(tsv.decode())
    got = open(out, "rb").read()
    assert got == want and got.count(b"\n") > 100
    assert not os.path.exists(out + ".partial")
    for dist, col in (("min_cont", 3), ("max_cont", 5)):
        engine.repr_sketches(tsv_path, dist, 0.30, out)
        assert open(out, "rb").read() == rr.repr_sketches(tsv.decode(), col, 0.30)
    # one pass, on one device and sharded over two engines
    p2 = str(other / "ix")
    for devices in (None, "0,0"):
        if devices:
            monkeypatch.setenv("KSPIDER_DEVICES", devices)
        engine.pairwise_and_repr(p2, 2, None, 0.20)
        assert open(p2 + "_kSpider_pairwise.tsv", "rb").read() == tsv
        assert open(p2 + "_kSpider_seqToKmersNo.tsv", "rb").read() == seq
        assert open(p2 + "_kSpider_repr_sketches.txt", "rb").read() == want
        for f in ("_kSpider_pairwise.tsv", "_kSpider_seqToKmersNo.tsv", "_kSpider_repr_sketches.txt"):
            os.remove(p2 + f)
    monkeypatch.delenv("KSPIDER_DEVICES")
    # the drop-in exe prints what the file holds
    run = subprocess.run([EXE, tsv_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stdout == want
    # a truncated line: KSP_E_IO naming the line, nothing left behind
    bad = str(tmp_path / "bad.tsv")
    lines = tsv.decode().split("\n")
    lines[10] = "\t".join(lines[10].split("\t")[:4])
    open(bad, "w").write("\n".join(lines))
    out2 = str(tmp_path / "never.txt")
    with pytest.raises(engine.KspError) as ei:
        engine.repr_sketches(bad, None, 0.20, out2)
    assert ei.value.code == engine.KSP_E_IO and "line 11" in str(ei.value)
    assert not os.path.exists(out2) and not os.path.exists(out2 + ".partial")
    lines[10] = "x" + tsv.decode().split("\n")[10]
    open(bad, "w").write("\n".join(lines))
    with pytest.raises(engine.KspError) as ei:
        engine.repr_sketches(bad, None, 0.20, out2)
    assert ei.value.code == engine.KSP_E_IO
    lines[10] = "-" + tsv.decode().split("\n")[10]
    open(bad, "w").write("\n".join(lines))
    with pytest.raises(engine.KspError) as ei:
        engine.repr_sketches(bad, None, 0.20, out2)
    assert ei.value.code == engine.KSP_E_ARG
    assert not os.path.exists(out2) and not os.path.exists(out2 + ".partial")
    for f in (lambda: engine.repr_sketches(tsv_path, "ani", 0.20, out2), lambda: engine.pairwise_and_repr(p2, 2, "ani", 0.20)):
        with pytest.raises(engine.KspError) as ei:
            f()
        assert ei.value.code == engine.KSP_E_ARG
    assert not os.path.exists(p2 + "_kSpider_pairwise.tsv")


@pytest.mark.parametrize("sub", ["plain", "nan"])
def test_pairwise_and_repr_with_rows_of_zero_weight_colours(oracle_lib, tmp_path, sub):
    """A row that exists only with shared_kmers = 0 (the pair 3-4 of tests/zero_weight_inputs.py; a NaN row when source 4 counts
    0 k-mers) is counted on the host after the device's ranking: it passes a negative threshold only (a NaN none).  The file of
    kspider_repr_sketches over the TSV of kspider_pairwise, and the restatement's."""
    import zero_weight_inputs
    prefix = str(tmp_path / "z")
    zero_weight_inputs.write(oracle_lib, prefix, sub)
    engine.pairwise(prefix, 1)
    tsv_path = prefix + "_kSpider_pairwise.tsv"
    tsv = open(tsv_path, "rb").read()
    assert any(r.split("\t")[:3] == ["3", "4", "0"] for r in tsv.decode().split("\n")[1:-1])
    out, fused = str(tmp_path / "two_steps.txt"), prefix + "_kSpider_repr_sketches.txt"
    seen = set()
    for dist, col in (("min_cont", 3), ("avg_cont", 4), ("max_cont", 5)):
        for threshold in (0.20, 0.0, -1.0):
            engine.repr_sketches(tsv_path, dist, threshold, out)
            want = open(out, "rb").read()
            assert want == rr.repr_sketches(tsv.decode(), col, threshold), (sub, dist, threshold)
            os.remove(tsv_path)
            engine.pairwise_and_repr(prefix, 1, dist, threshold)
            assert open(tsv_path, "rb").read() == tsv, (sub, dist, threshold)
            assert open(fused, "rb").read() == want, (sub, dist, threshold)
            os.remove(fused)
            seen.add(want)
            assert (b"3: 1\n" in want) == (threshold < 0 and sub == "plain"), (sub, dist, threshold)
    assert len(seen) >= 2

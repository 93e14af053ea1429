"""The containment cut on the GPU: a stable compaction of the join's edge records by the test `kSpider
cluster` applies, against the restatement in tests/cut_restate.py — every edge through the '%g' text of its own column value,
no critical float.  The output must equal edges[mask] record for record and in order, nothing behind it may be written, at
the sizes where a chunk (CUT_CHUNK_EDGES records) and a ballot (64 records) begin and end, with a grid so small that every
workgroup loops over chunks, and with the scatter pass reading the count pass's ballots or evaluating the predicate again."""
import functools
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cut_restate as cr
from kspider_amd import engine

pytestmark = pytest.mark.gpu

C = engine.CUT_CHUNK_EDGES
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "pairwise_cut")
SENTINEL = (0xDEADBEEF, 0xFEEDFACE, 0x0123456789ABCDEF)
TAIL = 5                       # sentinel records behind the last one the output could hold
N_NODES = 5200


def _edges(s1, s2, shared):
    e = np.zeros(len(s1), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = s1, s2, shared
    return e


def _sentinels(n):
    e = np.zeros(n, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = SENTINEL
    return e


def _device_cut(edges, kmer_counts, col, cutoff):
    """The kept records; asserts that everything behind them still holds the sentinel and that the input is unchanged."""
    n = len(edges)
    ed = engine.DeviceBuffer.from_numpy(edges) if n else None
    cd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(kmer_counts, dtype=np.uint32))
    od = engine.DeviceBuffer.from_numpy(_sentinels(n + TAIL))
    try:
        kept = engine.edges_cut(ed.ptr.value if ed else 0, n, cd.ptr.value, od.ptr.value, col, cutoff)
        out = od.to_numpy(engine.EDGE_DTYPE, n + TAIL)
        assert 0 <= kept <= n
        assert (out[kept:] == _sentinels(n + TAIL - kept)).all(), "a record behind n_kept was written"
        if n:
            assert (ed.to_numpy(engine.EDGE_DTYPE, n) == edges).all(), "d_edges was written"
        return out[:kept]
    finally:
        for b in (ed, cd, od):
            if b:
                b.free()


def _pattern_edges(n, mask):
    """n distinct records over sources of 1 000 k-mers each: containment 0.9 .. 0.949 where mask is set, 0.1 .. 0.149 elsewhere."""
    i = np.arange(n)
    return _edges(i // 4000, 1000 + i % 4000, np.where(mask, 900, 100) + i % 50)


def _masks(n):
    i = np.arange(n)
    edge = np.zeros(n, dtype=bool)      # only the last record of a chunk and the first of the next (the ends of the list when it is shorter)
    edge[[C - 1, C] if n > C else [0, n - 1] if n else []] = True
    return {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "alternating": i % 2 == 0, "chunk_edge": edge}


@pytest.mark.parametrize("ballots", [True, False])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17])
def test_patterns_at_ballot_and_chunk_boundaries(monkeypatch, n, ballots):
    if not ballots:
        monkeypatch.setenv("KSP_CUT_BALLOTS", "0")
    cnt = np.full(N_NODES, 1000, dtype=np.uint32)
    for name, mask in _masks(n).items():
        e = _pattern_edges(n, mask)
        for col in (3, 4, 5):
            want_mask = cr.edge_mask(e, cnt, col, 0.5)
            assert (want_mask == mask).all()                       # (the restatement agrees with how the case was built)
            got = _device_cut(e, cnt, col, 0.5)
            assert len(got) == int(mask.sum()) and (got == e[mask]).all(), (n, name, col, ballots)


@functools.lru_cache(maxsize=None)
def _random_case(n):
    """n records with values spread around 0.2 in all three columns (sources of 3 000 .. 4 000 k-mers), sorted by
    (source_1, source_2) and shuffled, with the masks the restatement gives for the cut 0.2."""
    rng = np.random.default_rng(n)
    cnt = rng.integers(3000, 4001, size=N_NODES).astype(np.uint32)
    i = np.arange(n)
    s1, s2 = i // 4000, 1000 + i % 4000
    u = rng.uniform(0.02, 0.4, size=n)
    shared = np.floor(u * 2.0 / (1.0 / cnt[s1] + 1.0 / cnt[s2])).astype(np.uint64)
    srt = _edges(s1, s2, shared)
    shuf = srt[rng.permutation(n)]
    masks = {}
    for name, e in (("sorted", srt), ("shuffled", shuf)):
        for col in (3, 4, 5):
            m = cr.edge_mask(e, cnt, col, 0.2)
            assert 0.3 < m.mean() < 0.7, (name, col, m.mean())
            masks[name, col] = m
    assert (masks["sorted", 3] != masks["sorted", 5]).any()          # the columns differ
    return {"sorted": srt, "shuffled": shuf}, cnt, masks


@pytest.mark.parametrize("ballots", [True, False])
def test_random_mask_sorted_and_shuffled_in_every_column(monkeypatch, ballots):
    if not ballots:
        monkeypatch.setenv("KSP_CUT_BALLOTS", "0")
    lists, cnt, masks = _random_case(3 * C + 17)
    for (name, col), m in masks.items():
        got = _device_cut(lists[name], cnt, col, 0.2)
        assert len(got) == int(m.sum()) and (got == lists[name][m]).all(), (name, col, ballots)


@pytest.mark.parametrize("ballots", [True, False])
def test_every_workgroup_loops_over_chunks(monkeypatch, ballots):
    """40 chunks (the last one short) on a grid of 3 workgroups: 13 or 14 chunks each."""
    monkeypatch.setenv("KSP_CUT_MAX_WORKGROUPS", "3")
    if not ballots:
        monkeypatch.setenv("KSP_CUT_BALLOTS", "0")
    lists, cnt, masks = _random_case(40 * C - 5)
    for name, col in (("shuffled", 4), ("sorted", 3)):
        m = masks[name, col]
        got = _device_cut(lists[name], cnt, col, 0.2)
        assert len(got) == int(m.sum()) and (got == lists[name][m]).all(), (name, col, ballots)


def _bits(v) -> int:
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


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
def test_boundary_floats(cutoff):
    """Sources of 2^24 k-mers: shared / 2^24 is exact for every float in [0.5, 1), so the critical float of the text test, its
    two neighbours and a NaN (no k-mers on either side, nothing shared) are the values of four records, in every column."""
    crit = _critical(cutoff)
    vals = [_float(crit - 1), _float(crit), _float(crit + 1)]
    assert vals[1] < np.float32(cutoff)                           # (a device comparing v >= cutoff would drop it)
    shared = [float(v) * 2.0**24 for v in vals]
    assert all(s == int(s) and 2**23 <= s < 2**24 for s in shared)
    cnt = np.array([2**24, 2**24, 0, 0, 7], dtype=np.uint32)
    e = _edges([0, 0, 0, 2, 2], [1, 1, 1, 3, 4], [int(s) for s in shared] + [0, 0])
    for col in (3, 4, 5):
        assert (cr.column_values(e[:3], cnt, col) == np.array(vals, dtype=np.float32)).all()
        want = cr.edge_mask(e, cnt, col, cutoff)
        assert want[:4].tolist() == [False, True, True, True], (col, want)     # below dropped; critical, above and NaN kept
        got = _device_cut(e, cnt, col, cutoff)
        assert (got == e[want]).all() and len(got) == int(want.sum()), (col, cutoff)


def test_refusals_leave_everything_untouched():
    e = _pattern_edges(100, np.ones(100, dtype=bool))
    ed = engine.DeviceBuffer.from_numpy(e)
    cd = engine.DeviceBuffer.from_numpy(np.full(N_NODES, 1000, dtype=np.uint32))
    od = engine.DeviceBuffer.from_numpy(_sentinels(100))
    try:
        E, K, O = ed.ptr.value, cd.ptr.value, od.ptr.value
        for args, kw in (((E, 100, K, O), dict(dist_col=2)), ((E, 100, K, O), dict(cutoff=float("nan"))), ((E, 100, K, E), {}),
                         ((E, 100, K, E + 16 * 99), {}), ((0, 100, K, O), {}), ((E, 100, 0, O), {}), ((E, 100, K, 0), {})):
            with pytest.raises(engine.KspError) as ei:
                engine.edges_cut(*args, **kw)
            assert ei.value.code == engine.KSP_E_ARG, (args, kw)
        assert (od.to_numpy(engine.EDGE_DTYPE, 100) == _sentinels(100)).all()
        assert (ed.to_numpy(engine.EDGE_DTYPE, 100) == e).all()
        assert engine.edges_cut(E, 100, K, O, 5, 0.5) == 100        # (the same buffers are fine when they do not overlap)
    finally:
        for b in (ed, cd, od):
            b.free()


# ---- files --------------------------------------------------------------------------------------------------------------

def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


def _sketches():
    from kspider_amd import synth
    return synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)   # (the index of tests/test_repr_gpu.py)


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The index, the full TSVs of engine.pairwise and the cuts to run: (dist, column, cut-off)."""
    d = tmp_path_factory.mktemp("cut")
    sk = _sketches()
    (d / "index").mkdir()
    index = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(index, sk.keys, sk.offsets)
    _names_map(index, sk.n_sources)
    shutil.copytree(d / "index", d / "a")
    prefix = str(d / "a" / "ix")
    engine.pairwise(prefix, 2)
    tsv = open(prefix + "_kSpider_pairwise.tsv", "rb").read()
    seq = open(prefix + "_kSpider_seqToKmersNo.tsv", "rb").read()
    rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
    assert len(rows) == 4342
    cuts = [("avg_cont", 4, 0.20)]
    for dist, col in (("min_cont", 3), ("max_cont", 5)):              # the printed value of the column's median row: a row's own text is the cut
        text = sorted((r[col] for r in rows), key=float)[len(rows) // 2]
        cuts.append((dist, col, float(text)))
    for dist, col, c in cuts:
        passing = sum(cr.keep(r[col], c) for r in rows)
        assert 0.05 * len(rows) <= passing <= 0.95 * len(rows), (dist, c, passing)
    return dict(dir=d, prefix=prefix, tsv=tsv, seq=seq, cuts=cuts)


def _cluster_file(prefix, dist, cutoff):
    engine.cluster(prefix, dist, cutoff)
    paths = glob.glob(prefix + "_kSpider_clusters_*")
    assert len(paths) == 1, paths
    data = open(paths[0], "rb").read()
    os.remove(paths[0])
    return os.path.basename(paths[0]), data


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_cut_tsv_is_the_filtered_full_tsv(full, monkeypatch, devices):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    prefix, tsv_path = full["prefix"], full["prefix"] + "_kSpider_pairwise.tsv"
    for dist, col, c in full["cuts"]:
        os.remove(tsv_path)
        engine.pairwise_cut(prefix, 2, dist, c)
        want = cr.cut_tsv(full["tsv"].decode(), col, c).encode()
        assert open(tsv_path, "rb").read() == want, (dist, c, devices)
        assert open(prefix + "_kSpider_seqToKmersNo.tsv", "rb").read() == full["seq"]
    engine.pairwise_cut(prefix, 2, "max_cont", 0.0)
    assert open(tsv_path, "rb").read() == full["tsv"]                 # a cut of 0 keeps every row


def test_clusters_over_the_cut_tsv_equal_those_over_the_full_tsv(full):
    prefix, tsv_path = full["prefix"], full["prefix"] + "_kSpider_pairwise.tsv"
    for dist, col, c in full["cuts"]:
        higher = min(1.0, c + 0.15)
        open(tsv_path, "wb").write(full["tsv"])
        want = [_cluster_file(prefix, dist, cc) for cc in (c, higher)]
        assert b"," in want[0][1] and want[0][1].count(b"\n") > 1           # (clusters of several members, and more than one cluster)
        os.remove(tsv_path)
        engine.pairwise_cut(prefix, 2, dist, c)
        assert len(open(tsv_path, "rb").read()) < len(full["tsv"])
        assert [_cluster_file(prefix, dist, cc) for cc in (c, higher)] == want, (dist, c)
    open(tsv_path, "wb").write(full["tsv"])


def test_exe_and_refusals(full):
    dist, col, c = full["cuts"][0]
    shutil.copytree(full["dir"] / "index", full["dir"] / "b")
    p2 = str(full["dir"] / "b" / "ix")
    before = sorted(os.listdir(full["dir"] / "b"))
    for d, cutoff in (("ani", 0.5), ("jaccard", 0.5), ("max_cont", 1.5), ("max_cont", -0.1), ("max_cont", float("nan"))):
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_cut(p2, 2, d, cutoff)
        assert ei.value.code == engine.KSP_E_ARG, (d, cutoff)
    assert sorted(os.listdir(full["dir"] / "b")) == before           # a refused call writes no file
    run = subprocess.run([EXE, p2, "2", dist, repr(c)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    assert open(p2 + "_kSpider_pairwise.tsv", "rb").read() == cr.cut_tsv(full["tsv"].decode(), col, c).encode()
    assert open(p2 + "_kSpider_seqToKmersNo.tsv", "rb").read() == full["seq"]
    run = subprocess.run([EXE, p2, "2", "ani", "0.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"ani" in run.stderr


def test_zero_weight_colours(oracle_lib, tmp_path):
    """Rows that exist only with shared_kmers = 0 are tested on the host.  Colours: {1, 2} weight 7; {3, 4} weight 0 (the
    pair shares nothing else); {5, 6} weight 0 AND {5, 6} weight 1 (a real row of a pair that is also a zero pair)."""
    co = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
    src = np.array([1, 2, 3, 4, 5, 6, 5, 6], dtype=np.uint32)
    w = np.array([7, 0, 0, 1], dtype=np.uint32)
    ids = np.arange(1, 7, dtype=np.uint32)

    def run(sub, counts, dist, col, c):
        d = tmp_path / sub
        d.mkdir()
        prefix = str(d / "z")
        oracle_lib.write_index(prefix, co, src, w, ids, np.array(counts))
        engine.pairwise(prefix, 1)
        whole = open(prefix + "_kSpider_pairwise.tsv").read()
        os.remove(prefix + "_kSpider_pairwise.tsv")
        engine.pairwise_cut(prefix, 1, dist, c)
        got = open(prefix + "_kSpider_pairwise.tsv").read()
        assert got == cr.cut_tsv(whole, col, c), (sub, whole, got)
        return whole, got

    whole, got = run("cut0", [10, 20, 30, 40, 50, 60], "max_cont", 5, 0.0)
    assert got == whole and "\n3\t4\t0\t0\t0\t0\n" in got
    whole, got = run("cut05", [10, 20, 30, 40, 50, 60], "max_cont", 5, 0.5)
    assert "\n3\t4\t" not in got and "\n1\t2\t7\t" in got and "\n5\t6\t" not in got
    # a source of 0 k-mers: the row of the zero pair is a NaN row, and kept
    whole, got = run("nan", [10, 20, 30, 0, 50, 60], "max_cont", 5, 0.5)
    assert "\n3\t4\t0\t" in got and "nan" in got
    # ... but a pair whose real row (1 shared k-mer, min containment 1 / 50) the device dropped gets no NaN row in its place
    whole, got = run("dropped", [10, 20, 30, 0, 50, 0], "min_cont", 3, 0.5)
    assert "\n5\t6\t1\t" in whole and "\n5\t6\t" not in got and "\n3\t4\t0\t" in got


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_host_buffer_form(devices):
    sk = _sketches()
    whole, _ = engine.pairwise_host(sk.keys, sk.offsets)
    lengths = np.diff(sk.offsets.astype(np.int64)).astype(np.uint32)
    for counts, col, c in ((None, 4, 0.20), (None, 5, 0.25), (lengths * 2 + 1, 3, 0.1)):
        mask = cr.edge_mask(whole, lengths if counts is None else counts, col, c)
        assert 0.05 < mask.mean() < 0.95, (col, c, mask.mean())
        got, n_found, st = engine.pairwise_host_cut(sk.keys, sk.offsets, kmer_counts=counts, dist_col=col, cutoff=c, devices=devices)
        assert (got == whole[mask]).all() and len(got) == int(mask.sum()), (devices, col, c)
        assert n_found == len(whole) and st["last_edges"] == len(got)
    got, n_found, _ = engine.pairwise_host_cut(sk.keys, sk.offsets, cutoff=0.0, devices=devices)
    assert (got == whole).all() and n_found == len(whole)
    got, n_found, _ = engine.pairwise_host_cut(sk.keys, sk.offsets, dist_col=3, cutoff=2.0, devices=devices)   # nothing passes
    assert len(got) == 0 and n_found == len(whole)

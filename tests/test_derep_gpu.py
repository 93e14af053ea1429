"""Dereplication on the GPU against the restatement in tests/derep_restate.py: rep, via, rank, degree and the
number of representatives compared element for element, plus the four consequences of the definition.  Paths that need
hundreds of rounds, with the single-workgroup tail and without it; the tail's switch at exactly KSP_DEREP_TAIL_PAIRS live
pairs; a representative of smaller rank that is decided later than the one that knocks the node out; stars, a clique,
isolated nodes, self pairs, an endpoint out of range; the boundary floats of the text test; the sizes where a ballot and a
chunk begin and end and a grid so small that every workgroup loops; random graphs on both sides of the counting kernel's
LDS switch; seeded multigraphs (tests/derep_inputs.hostile: repeated pairs in both orientations, self pairs, ends out of range, nodes
of 0 k-mers, tied stars) in two sizes, every column, both round modes and a second record order; the join's own records and the
file-writing calls on a 400-source index; a pairwise TSV written by hand.  Every output array has sentinels behind
it and d_edges is compared after every call.  The inputs come from tests/derep_inputs.py, whose shapes
tests/test_derep_cpu.py checks without a GPU."""
import functools
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import derep_inputs as di
import derep_restate as dr
import repr_restate as rr
from kspider_amd import engine

pytestmark = pytest.mark.gpu

C = engine.DEREP_CHUNK_EDGES
K = engine.DEREP_TAIL_PAIRS
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "dereplicate")
TAIL = 7                        # sentinel entries behind every output array
FILL = 0xDEADBEEF
KEYS = ("rep", "via", "rank", "degree")


def _device(n_nodes, e, cnt, col=4, threshold=0.20):
    """ksp_edges_dereplicate over e; returns (result, what the rounds did)."""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    ed = engine.DeviceBuffer.from_numpy(e) if len(e) else None
    cd = engine.DeviceBuffer.from_numpy(cnt)
    try:
        got = engine.edges_dereplicate(n_nodes, ed.ptr.value if ed else 0, len(e), cd.ptr.value, col, threshold, tail=TAIL, fill=FILL)
        if len(e):
            assert (ed.to_numpy(engine.EDGE_DTYPE, len(e)) == e).all(), "d_edges was written"
        return got, engine.derep_rounds()
    finally:
        for buf in (ed, cd):
            if buf:
                buf.free()


def _same_as(got, want, what=None):
    for k in KEYS:
        assert (got[k] == want[k]).all(), (what, k, int((got[k] != want[k]).sum()))
    assert got["n_reps"] == want["n_reps"], what


def _check(n_nodes, e, cnt=None, col=4, threshold=0.20, want=None):
    cnt = di.same(n_nodes) if cnt is None else cnt
    want = dr.dereplicate(e, cnt, col, threshold, n_nodes) if want is None else want
    got, rounds = _device(n_nodes, e, cnt, col, threshold)
    _same_as(got, want, (n_nodes, len(e), col))
    return got, rounds


# ---- rounds: paths, the tail and its switch ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["ascending", "reversed", "random"])
def test_paths_of_300_with_and_without_the_tail(monkeypatch, order):
    e = di.path(300, order, seed=5)
    want = dr.dereplicate(e, di.same(300), 4, 0.20, 300)
    assert want["n_reps"] == 150                                       # the odd nodes 1 .. 297, and the end 299 behind the member 298
    got, r = _check(300, e, want=want)
    assert r["dispatched"] == 1 and r["tail"] > 100 and r["live_at_tail"] == 299 and r["kept"] == 299, r
    monkeypatch.setenv("KSP_DEREP_TAIL", "0")
    got0, r0 = _check(300, e, want=want)
    assert r0["dispatched"] > 100 and r0["tail"] == 0, r0
    _same_as(got0, got)


@functools.lru_cache(maxsize=None)
def _paths_case(total):
    n, e = di.disjoint_paths(total)
    return n, e, dr.dereplicate(e, di.same(n), 4, 0.20, n)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tail_switch_at_exactly_the_constant(delta):
    """Disjoint paths with K - 1, K and K + 1 records: every pair is live after the first round, so the tail takes over after
    round 1 with all of them — or, one pair above the constant, only after a later round has let pairs die."""
    n, e, want = _paths_case(K + delta)
    got, r = _check(n, e, want=want)
    assert r["kept"] == K + delta and r["tail"] > 0, r
    if delta <= 0:
        assert r["dispatched"] == 1 and r["live_at_tail"] == K + delta, r
    else:
        assert r["dispatched"] >= 2 and r["live_at_tail"] <= K, r


def test_tail_and_host_rounds_agree_on_the_switch_graph(monkeypatch):
    n, e, want = _paths_case(K + 1)
    monkeypatch.setenv("KSP_DEREP_TAIL", "0")
    got, r = _check(n, e, want=want)
    assert r["tail"] == 0 and r["dispatched"] >= 4, r


# ---- assignment ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", ["1", "0"])
def test_a_smaller_ranked_representative_decided_later_gets_the_node(monkeypatch, tail):
    monkeypatch.setenv("KSP_DEREP_TAIL", tail)
    n, e = di.later_smaller_rep()
    L = di.LATER
    got, r = _check(n, e)
    assert got["rep"][L["h"]] == L["u2"] and got["via"][L["h"]] == 1 and got["rep"][L["u1"]] == L["u1"]
    assert r["dispatched"] + r["tail"] >= 2
    # the pair 0 - 1 three times with different `shared`, the first one not kept: via is the lowest kept index
    e = di.edges([0, 1, 0, 0], [1, 0, 1, 2], [di.DROP, di.KEEP, di.KEEP + 5, di.KEEP])
    got, _ = _check(3, e)
    assert got["via"].tolist() == [dr.NONE, 1, 3] and got["degree"].tolist() == [3, 2, 1]


# ---- shapes ----------------------------------------------------------------------------------------------------------------------

def test_star_clique_isolated_self_pairs_and_out_of_range():
    for centre_first in (True, False):
        got, _ = _check(5001, di.star(5000, centre_first))
        assert got["n_reps"] == 1 and (got["rep"] == 0).all()
    got, _ = _check(200, di.clique(200))
    assert got["n_reps"] == 1 and (got["rep"] == 0).all() and (got["degree"] == 199).all()
    # 1 000 isolated nodes and no record: no kernel runs, all are representatives, ranked in node order
    got, r = _check(1000, di.edges([], []))
    assert got["n_reps"] == 1000 and (got["rank"] == np.arange(1000)).all() and r == dict(dispatched=0, tail=0, live_at_tail=0, kept=0)
    # the same when not even +inf passes
    got, r = _check(300, di.path(300), threshold=float("inf"))
    assert got["n_reps"] == 300 and r["dispatched"] == 0
    # self pairs only: degrees, no pair
    got, r = _check(3, di.edges([1, 2, 2], [1, 2, 2]))
    assert got["degree"].tolist() == [0, 2, 4] and got["n_reps"] == 3 and got["rank"].tolist() == [2, 1, 0] and r["kept"] == 0 and r["dispatched"] == 1
    got, _ = _check(3, di.edges([2, 2, 0, 2], [2, 2, 1, 1]))
    assert got["rep"].tolist() == [0, 2, 2]
    # an endpoint >= n_nodes is ignored, whichever end it is
    got, r = _check(3, di.edges([0, 1, 9, 1], [7, 2, 1, 0xFFFFFFFF]))
    assert got["degree"].tolist() == [0, 1, 1] and got["rep"].tolist() == [0, 1, 1] and r["kept"] == 1


@pytest.mark.parametrize("col", [3, 4, 5])
def test_boundary_floats_of_the_text_test(col):
    """At 0.20: 0.1999996 prints "0.2" and passes (a device comparing v > 0.2 fails here), 0.1999994 prints "0.199999" and fails,
    a NaN fails; the ends of every record count different numbers of k-mers."""
    cnt, e = di.boundary_case(col)
    got, r = _check(8, e, cnt, col)
    assert got["degree"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and got["rep"].tolist() == [0, 0, 2, 3, 4, 5, 6, 6] and r["kept"] == 2


# ---- sizes -----------------------------------------------------------------------------------------------------------------------

N_NODES = 5200


def _random_case(n, seed, n_nodes=N_NODES):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(3000, 4001, size=n_nodes).astype(np.uint32)
    s1, s2 = rng.integers(0, n_nodes, size=n), rng.integers(0, n_nodes, size=n)
    shared = (rng.uniform(0.02, 0.4, size=n) * 2.0 / (1.0 / cnt[s1] + 1.0 / cnt[s2])).astype(np.uint64)
    return di.edges(s1, s2, shared), cnt


@pytest.mark.parametrize("n", [1, 63, 64, 65, C - 1, C, C + 1])
def test_ballot_and_chunk_boundaries(n):
    e, cnt = _random_case(n, 100 + n)
    for col in (3, 4, 5):
        got, r = _check(N_NODES, e, cnt, col)
    if n >= C - 1:
        assert 0 < r["kept"] < n


@pytest.mark.parametrize("tail", ["1", "0"])
def test_every_workgroup_loops_over_chunks(monkeypatch, tail):
    """40 chunks (the last one short) on a grid of 3 workgroups: 13 or 14 chunks each, in every edge pass."""
    monkeypatch.setenv("KSP_DEREP_MAX_WORKGROUPS", "3")
    monkeypatch.setenv("KSP_DEREP_TAIL", tail)
    e, cnt = _random_case(40 * C - 5, 40)
    got, r = _check(N_NODES, e, cnt)
    assert r["kept"] > 10 * C and (r["tail"] > 0) == (tail == "1"), r
    kept = np.array(dr.kept_records(e, cnt, 4, 0.20, N_NODES), dtype=np.int64)
    di.consequences(N_NODES, e, kept, got)


@functools.lru_cache(maxsize=None)
def _lds_case(n_nodes):
    e, cnt = _random_case(50_000, n_nodes, n_nodes)
    srt = e[np.lexsort((e["source_2"], e["source_1"]))]
    shuf, _ = di.permuted(srt, n_nodes)
    return srt, shuf, cnt


@pytest.mark.parametrize("n_nodes", [16383, 16384, 16385])
def test_random_graphs_on_both_sides_of_the_lds_switch(n_nodes):
    srt, shuf, cnt = _lds_case(n_nodes)
    seen = []
    for name, e in (("sorted", srt), ("shuffled", shuf)):
        got, r = _check(n_nodes, e, cnt)
        kept = np.array(dr.kept_records(e, cnt, 4, 0.20, n_nodes), dtype=np.int64)
        assert len(e) / 3 < len(kept) == r["kept"] + int((e["source_1"][kept] == e["source_2"][kept]).sum()) < 2 * len(e) / 3
        di.consequences(n_nodes, e, kept, got)
        seen.append(got)
    for k in ("rep", "rank", "degree"):                       # only via depends on the order of the records
        assert (seen[0][k] == seen[1][k]).all(), k


@functools.lru_cache(maxsize=None)
def _hostile_case(n_nodes, n_records):
    e, cnt, _ = di.hostile(11, n_nodes, n_records)
    e2, _ = di.permuted(e, 3)
    want = {(k, col): dr.dereplicate(ee, cnt, col, 0.20, n_nodes) for k, ee in enumerate((e, e2)) for col in (3, 4, 5)}
    kept2 = {col: dr.kept_records(e2, cnt, col, 0.20, n_nodes) for col in (3, 4, 5)}
    return e, e2, cnt, want, kept2


@pytest.mark.parametrize("tail", ["1", "0"])
@pytest.mark.parametrize("n_nodes,n_records", [(700, 3 * C - 7), (20000, 2 * C + 1)])
def test_hostile_multigraphs(monkeypatch, n_nodes, n_records, tail):
    """Dense on 700 nodes (several rounds) and beyond the counting kernel's LDS switch on 20 000; with the tail, and with host-driven
    rounds on a grid of 2 workgroups.  The 64-bit atomicMin of (rank, index) decides among 2 .. 6 copies of a pair whose first
    copy is often dropped; what tests/test_derep_cpu.py shows about the inputs holds for the restatement alone."""
    monkeypatch.setenv("KSP_DEREP_TAIL", tail)
    if tail == "0":
        monkeypatch.setenv("KSP_DEREP_MAX_WORKGROUPS", "2")
    e, e2, cnt, want, kept2 = _hostile_case(n_nodes, n_records)
    for col in (3, 4, 5):
        got, r = _check(n_nodes, e, cnt, col, want=want[0, col])
        assert (r["tail"] > 0) == (tail == "1") and r["dispatched"] >= 1, r
        got2, _ = _check(n_nodes, e2, cnt, col, want=want[1, col])
        di.consequences(n_nodes, e2, np.array(kept2[col], dtype=np.int64), got2)
        di.via_after_permutation(e2, kept2[col], got, got2)


def test_rank_of_the_nodes_with_a_neighbour_is_the_order_of_edges_repr():
    e, cnt = _random_case(3000, 7, 1000)
    ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
    try:
        node, count = engine.edges_repr(1000, ed.ptr.value, len(e), cd.ptr.value, 4, 0.20)
        got = engine.edges_dereplicate(1000, ed.ptr.value, len(e), cd.ptr.value, 4, 0.20, tail=TAIL, fill=FILL)
    finally:
        ed.free()
        cd.free()
    assert 0 < len(node) < 1000
    assert got["rank"][node].tolist() == list(range(len(node))) and (got["degree"][node] == count).all()
    rest = np.setdiff1d(np.arange(1000), node)
    assert got["rank"][rest].tolist() == list(range(len(node), 1000)) and (got["degree"][rest] == 0).all()


# ---- the join's own records and the files ----------------------------------------------------------------------------------------

DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The 400-source index of tests/test_repr_gpu.py with a .namesMap, the TSVs of engine.pairwise and the join's records."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("derep")
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
    edges, _ = engine.pairwise_host(sk.keys, sk.offsets)
    return dict(dir=d, prefix=prefix, tsv=_read(prefix + "_kSpider_pairwise.tsv"), seq=_read(prefix + "_kSpider_seqToKmersNo.tsv"), names=names,
                edges=edges, sizes=sk.sizes.astype(np.uint32), n=sk.n_sources)


def test_join_records_at_four_thresholds(full):
    e, cnt, n = full["edges"], full["sizes"], full["n"]
    row = full["tsv"].decode().split("\n")[len(e) // 2].split("\t")
    reps = set()
    for col in (3, 4, 5):
        for threshold in (0.0, 0.20, 0.5, float(row[col])):
            got, r = _check(n, e, cnt, col, threshold)
            di.consequences(n, e, np.array(dr.kept_records(e, cnt, col, threshold, n), dtype=np.int64), got)
            reps.add(got["n_reps"])
    assert len(reps) >= 3 and min(reps) < n / 2


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_files_from_hbm_and_from_the_tsv_are_byte_equal(full, monkeypatch, devices):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    for dist, col in DISTS.items():
        threshold = 0.20 if dist == "avg_cont" else 0.35
        want = dr.dereplicated_tsv(full["tsv"].decode(), full["names"], col, threshold, dist)
        assert want.count(b"\t-\t") not in (0, full["n"])
        d = full["dir"] / f"fused_{dist}_{devices}"
        shutil.copytree(full["dir"] / "index", d)
        fused = str(d / "ix")
        engine.pairwise_and_dereplicate(fused, 2, None if dist == "avg_cont" else dist, threshold)
        assert _read(fused + "_kSpider_pairwise.tsv") == full["tsv"] and _read(fused + "_kSpider_seqToKmersNo.tsv") == full["seq"], (dist, devices)
        out = fused + f"_kSpider_dereplicated_{dist}.tsv"
        from_hbm = _read(out)
        os.remove(out)
        engine.dereplicate(fused, dist, threshold)
        assert from_hbm == _read(out) == want, (dist, devices)
        assert not glob.glob(str(d / "*.partial"))


def test_exe_and_refusals(full):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    out = str(d / "mine.tsv")
    run = subprocess.run([EXE, prefix, "max_cont", "0.5", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    assert _read(out) == dr.dereplicated_tsv(full["tsv"].decode(), full["names"], 5, 0.5, "max_cont")
    os.remove(out)
    before = sorted(os.listdir(d))
    nan = float("nan")
    for call in (lambda: engine.dereplicate(prefix, "ani", 0.2), lambda: engine.pairwise_and_dereplicate(prefix, 1, "ani", 0.2),
                 lambda: engine.dereplicate(prefix, None, nan), lambda: engine.pairwise_and_dereplicate(prefix, 1, None, nan),
                 lambda: engine.dereplicate(prefix, None, -0.5), lambda: engine.pairwise_and_dereplicate(prefix, 1, None, -0.5),
                 lambda: engine.dereplicate(prefix, "jaccard", 0.2),
                 lambda: engine.edges_dereplicate(4, 0, 5, 0, 4), lambda: engine.edges_dereplicate(4, 0, 0, 0, 6),
                 lambda: engine.edges_dereplicate(4, 0, 0, 0, 4, nan)):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    run = subprocess.run([EXE, prefix, "ani", "0.2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"ani" in run.stderr
    assert sorted(os.listdir(d)) == before
    # an id missing from .namesMap: the TSV path refuses the passing row that names it, the fused call the source
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.dereplicate(prefix, None, 0.2)
    assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value) and sorted(os.listdir(d)) == before
    os.remove(prefix + "_kSpider_pairwise.tsv")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise_and_dereplicate(prefix, 1, None, 0.2)
    assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(d)) == before


HAND_ROWS = (                       # source_1, source_2, shared_kmers, min, avg, max: all three columns carry the row's value
    ("2", "1", "0.1"),              # the pair 1 - 2 three times, both orientations, the failing value first
    ("1", "2", "0.200001"),
    ("2", "1", "inf"),
    ("3", "3", "0.5"),              # two self rows, one passes
    ("4", "4", "1e-1"),
    ("3", "4", "nan"),
    ("4", "3", "-nan"),
    ("5", "3", "0.2"),              # reads as 0.2f, above 0.20
    ("5", "1", "0.200001 "),        # a blank behind the value
    ("6", "5", "inf"),
    ("6", "2", "0.3"),
    ("9", "1", "0.1"),              # fails: the id beyond .namesMap is never looked at
)


def test_a_tsv_no_writer_of_ours_produced(tmp_path):
    prefix = str(tmp_path / "hand")
    names = [f"g{i}" for i in range(1, 8)]
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {n}\n" for i, n in enumerate(names)))
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n" + "".join(f"{i + 1}\t{i + 1}\t{100 + i}\n" for i in range(len(names))))
    text = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n" + \
           "".join(f"{a}\t{b}\t7\t{v}\t{v}\t{v}\n" for a, b, v in HAND_ROWS)
    assert len(HAND_ROWS) == 12
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write(text)
    for dist, col in DISTS.items():
        want = dr.dereplicated_tsv(text, names, col, 0.20, dist)
        engine.dereplicate(prefix, dist, 0.20)
        assert _read(prefix + f"_kSpider_dereplicated_{dist}.tsv") == want, dist
    # by hand: 1 has the rows to 2 (twice), 5; 5 has 3, 1, 6; 2 has 1 (twice), 6; 3 has its self row (2) and 5; 6 has 5, 2
    rows = [l.split("\t") for l in want.decode().split("\n")[1:-1]]
    assert [r[3] for r in rows] == ["3", "3", "3", "0", "3", "2", "0"]
    assert [r[4] for r in rows] == ["0", "1", "2", "5", "3", "4", "6"]
    assert [r[1] for r in rows] == ["g1", "g1", "g3", "g4", "g1", "g6", "g7"] and rows[1][2] == "0.200001" and rows[4][2] == "0.200001"

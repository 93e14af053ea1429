"""The cluster report on the GPU against the restatement in tests/report_restate.py: both tables compared for exact
equality, at the default grid and at KSP_REPORT_MAX_WORKGROUPS=1.  The sizes where a ballot and a chunk begin and end; runs of one
source_1 across waves and chunks, one label over several chunks with what ksp_debug_report_counts reports, and the same records
shuffled among other clusters; one hostile multigraph in three orders; ties; NaN records, self pairs, ends out of range, repeated
pairs, records of value 0; the cut-off boundary; the quantisation and a strength above 2^53; the domain refusal; host edges; every
refusal; and the file-writing calls on a 400-source index, on one and on two workers, with the device's row text, on colours of
weight 0, the executable.  Every output array has sentinels behind it and d_edges is compared after every call.  The inputs come
from tests/report_inputs.py, whose properties tests/test_report_cpu.py checks without a GPU."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import report_inputs as ri
import report_restate as rs
import repr_restate as rr
import zero_weight_inputs as zw
from kspider_amd import engine

pytestmark = pytest.mark.gpu

C = engine.REPORT_CHUNK_EDGES
NONE = rs.NONE
TAIL = 5                        # sentinel rows behind both output arrays
FILL = 0xA5
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "cluster_report")
DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


def _device(n_nodes, e, cnt, col, cutoff):
    """ksp_edges_cluster_report over e; returns ((cluster, member), what the passes did)."""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    ed = engine.DeviceBuffer.from_numpy(e) if len(e) else None
    cd = engine.DeviceBuffer.from_numpy(cnt)
    try:
        try:
            got = engine.edges_cluster_report(n_nodes, ed.ptr.value if ed else 0, len(e), cd.ptr.value, col, cutoff, tail=TAIL, fill=FILL)
        finally:
            if len(e):
                assert (ed.to_numpy(engine.EDGE_DTYPE, len(e)) == e).all(), "d_edges was written"
        return got, engine.report_counts()
    finally:
        for buf in (ed, cd):
            if buf:
                buf.free()


def _check(monkeypatch, n_nodes, e, cnt, col, cutoff, caps=(None, 1), want=None):
    """The call at every grid cap (None: the default grid) against the restatement; returns (the restatement's result, the counts
    per cap)."""
    want = rs.report_edges(e, cnt, col, cutoff, n_nodes) if want is None else want
    seen = {}
    for cap in caps:
        if cap is None:
            monkeypatch.delenv("KSP_REPORT_MAX_WORKGROUPS", raising=False)
        else:
            monkeypatch.setenv("KSP_REPORT_MAX_WORKGROUPS", str(cap))
        got, seen[cap] = _device(n_nodes, e, cnt, col, cutoff)
        rs.same(got, want, (cap, n_nodes, len(e), col, cutoff))
        assert seen[cap]["kept"] == int(want[0]["edges"].sum())
    monkeypatch.delenv("KSP_REPORT_MAX_WORKGROUPS", raising=False)
    return want, seen


# ---- 1. sizes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ri.PATH_SIZES)
def test_ballot_and_chunk_boundaries_on_a_path(monkeypatch, n):
    e, cnt, n_nodes = ri.path_case(n)
    caps = (None, 1, 2) if n == 2 * C + 1 else (None, 1)                      # 3 chunks on 2 workgroups: a workgroup loops
    want, seen = _check(monkeypatch, n_nodes, e, cnt, 5, 0.0, caps)
    assert want[0]["size"].tolist() == [n_nodes] and want[0]["edges"].tolist() == [n]
    for cap in caps:
        assert seen[cap]["single_label_chunks"] == -(-n // C) == seen[cap]["cluster_sets"], seen   # one label: one set per chunk
        assert seen[cap]["node_sets"] == n                                    # a path: every source_1 is a run of its own


# ---- 2. runs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre_first", [True, False])
def test_a_star_of_5000_leaves(monkeypatch, centre_first):
    e, cnt, n_nodes = ri.star_case(centre_first)
    want, seen = _check(monkeypatch, n_nodes, e, cnt, 4, 0.0)
    assert want[0]["medoid"].tolist() == [0] and want[0]["covered"].tolist() == [5000] and int(want[1]["strength"][0]) == 5000 << 31
    for counts in seen.values():
        # the centre as source_1: one run per ballot of 64 lanes, 79 of them; as source_2: every record is its own run
        assert counts["node_sets"] == (-(-5000 // 64) if centre_first else 5000), counts
        assert counts["single_label_chunks"] == counts["cluster_sets"] == 3


def test_a_clique_of_70_is_one_label_over_two_chunks(monkeypatch):
    e, cnt, n_nodes = ri.clique_case()
    chunks = -(-len(e) // C)
    want, seen = _check(monkeypatch, n_nodes, e, cnt, 3, 0.0)
    assert chunks == 2 and want[0]["edges"].tolist() == [2415] and want[0]["medoid"].tolist() == [0] and want[0]["covered"].tolist() == [69]
    for counts in seen.values():
        assert counts["single_label_chunks"] == chunks and counts["cluster_sets"] <= chunks, counts


def test_the_clique_shuffled_among_ten_paths(monkeypatch):
    e, cnt, n_nodes, part = ri.clique_and_paths()
    want, seen = _check(monkeypatch, n_nodes, e, cnt, 5, 0.0)
    alone = rs.report_edges(ri.clique_case()[0], ri.clique_case()[1], 5, 0.0, 70)
    big = want[0][want[0]["root"] == 0]
    assert big.tolist() == alone[0].tolist()                                  # the clique's row is what it was
    for field in ("label", "degree", "strength"):
        assert (want[1][field][:70] == alone[1][field]).all()
    assert (want[1]["via"][:70] != alone[1]["via"]).any()                     # via follows the indices
    first = {}
    for i, (a, b) in enumerate(zip(e["source_1"].tolist(), e["source_2"].tolist())):
        first.setdefault((min(a, b), max(a, b)), i)
    assert want[1]["via"][1:70].tolist() == [first[0, v] for v in range(1, 70)]
    for counts in seen.values():
        assert counts["single_label_chunks"] == 0 and counts["cluster_sets"] > 80   # mixed labels: sets per run and wave


# ---- 3. order independence -------------------------------------------------------------------------------------------------------

def test_hostile_multigraph_in_three_orders(monkeypatch):
    e, cnt, _ = ri.hostile()
    results = {}
    for name, eo in ri.orders(e).items():
        results[name], _ = _check(monkeypatch, 20000, eo, cnt, 4, 0.2)
    base = results["ascending"]
    assert len(base[0]) < 20000 and int(base[0]["nan_edges"].sum()) > 0 and int(base[0]["size"].max()) > 5
    for name in ("reversed", "shuffled"):
        rs.same(results[name], base, name, via=False)
        assert (results[name][1]["via"] != base[1]["via"]).any()
    for col in (3, 5):
        _check(monkeypatch, 20000, e, cnt, col, 0.2, caps=(None,))


# ---- 4. ties and specials --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ri.SMALL))
def test_small_graphs_in_every_column(monkeypatch, name):
    n, a, b, v, _ = ri.SMALL[name]
    want = rs.report(n, a, b, v)
    e, cnt, n_nodes = ri.small_records(name)
    for col in (3, 4, 5):
        _check(monkeypatch, n_nodes, e, cnt, col, 0.0, want=want)


@pytest.mark.parametrize("col", [3, 4, 5])
def test_specials(monkeypatch, col):
    e, cnt, n, notes = ri.specials()
    for cutoff, zero_kept in ((0.0, True), (0.2, False)):
        (cluster, member), _ = _check(monkeypatch, n, e, cnt, col, cutoff)
        assert (member["label"][[9, 10, 11]].tolist() == [9, 9, 9]) == zero_kept
        nan = cluster[cluster["root"] == 6][0]
        assert nan["size"] == 3 and nan["edges"] == nan["nan_edges"] == 2 and np.isnan(nan["min"]) and nan["medoid"] == 6
        assert member["degree"][0] == 3 and member["degree"][2] == 1 and member["degree"][3] == 1


def test_cutoff_boundary(monkeypatch):
    e, cnt, cutoff = ri.boundary()
    for col in (3, 4, 5):
        (cluster, member), _ = _check(monkeypatch, 4, e, cnt, col, cutoff)
        assert member["label"].tolist() == [0, 0, 2, 3] and cluster["edges"].tolist() == [1, 0, 0]


# ---- 5. quantisation and the domain ----------------------------------------------------------------------------------------------

def test_quantisation(monkeypatch):
    e, cnt = ri.quantised()
    (cluster, member), _ = _check(monkeypatch, 4, e, cnt, 3, 0.0)
    assert int(member["strength"][0]) == 1 << 12 == int(cluster["sum_q"][0])
    v = np.float32(1) / np.float32(3072)
    assert int(member["strength"][2]) == rs.q_exact(v) and int(member["strength"][2]) * 2.0**-32 < float(v)


def test_a_strength_above_2_to_the_53(monkeypatch):
    e, cnt, n = ri.heavy()
    (cluster, member), _ = _check(monkeypatch, n, e, cnt, 5, 0.0, caps=(None,))
    assert int(member["strength"][0]) == 3_000_000 << 32 > 1 << 53 and int(cluster["sum_q"][0]) == 3_000_000 << 32
    assert member["degree"].tolist() == [3_000_000] * 2 and member["via"].tolist() == [NONE, 0]


def test_domain(monkeypatch):
    e, cnt = ri.out_of_domain()
    for cap in (None, 1):
        if cap:
            monkeypatch.setenv("KSP_REPORT_MAX_WORKGROUPS", str(cap))
        for col in (3, 4, 5):
            with pytest.raises(engine.KspError) as ei:                        # (the wrapper checks every output byte after a refusal)
                _device(4, e, cnt, col, 0.0)
            assert ei.value.code == engine.KSP_E_ARG and "[0, 1]" in str(ei.value)
    _check(monkeypatch, 4, e, cnt, 5, 2.0)                                    # below the cut-off: not kept, no refusal
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report_valued(4, [0, 2], [1, 3], [0.5, 1.5], tail=TAIL, fill=FILL)
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report_valued(4, [0, 2], [1, 3], [0.5, float("inf")], tail=TAIL, fill=FILL)
    assert ei.value.code == engine.KSP_E_ARG


# ---- 6. host edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["hostile", "specials"])
def test_valued_host_edges(monkeypatch, which):
    if which == "hostile":
        e, cnt, _ = ri.hostile()
        n, cutoff = 20000, 0.2
    else:
        e, cnt, n, _ = ri.specials()
        cutoff = 0.0
    k = np.nonzero(rs.kept_mask(e, cnt, 4, cutoff, n))[0]
    v = rr.column_values(e[k], cnt, 4)
    want = rs.report(n, e["source_1"][k], e["source_2"][k], v)
    for cap in (None, 1):
        if cap:
            monkeypatch.setenv("KSP_REPORT_MAX_WORKGROUPS", str(cap))
        rs.same(engine.cluster_report_valued(n, e["source_1"][k], e["source_2"][k], v, tail=TAIL, fill=FILL), want, (which, cap))
    monkeypatch.delenv("KSP_REPORT_MAX_WORKGROUPS")
    from_records, _ = _device(n, e, cnt, 4, cutoff)                            # the same rows as the records give, via apart
    rs.same(from_records, want, which, via=False)
    wv = want[1]["via"].astype(np.int64)
    assert (from_records[1]["via"] == np.where(wv == NONE, NONE, k[np.minimum(wv, len(k) - 1)])).all()   # the kept record's own index


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_and_no_records(monkeypatch):
    e, cnt, n = ri.small_records("path3")
    ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
    L = engine.lib()
    out_c, out_m, out_n = np.zeros(4, dtype=engine.CLUSTER_ROW_DTYPE), np.zeros(4, dtype=engine.MEMBER_ROW_DTYPE), np.zeros(1, dtype=np.uint32)
    pc, pm, pn = out_c.ctypes.data, out_m.ctypes.data, out_n.ctypes.data
    try:
        arg = [
            lambda: engine.edges_cluster_report(n, 0, 2, cd.ptr.value, 5, 0.0, tail=TAIL, fill=FILL),                 # NULL edges, n_edges > 0
            lambda: engine.edges_cluster_report(n, ed.ptr.value, 2, 0, 5, 0.0, tail=TAIL, fill=FILL),                 # NULL counts
            lambda: engine.edges_cluster_report(n, ed.ptr.value, 2, cd.ptr.value, 6, 0.0, tail=TAIL, fill=FILL),      # the column
            lambda: engine.edges_cluster_report(n, ed.ptr.value, 2, cd.ptr.value, 2, 0.0, tail=TAIL, fill=FILL),
            lambda: engine.edges_cluster_report(n, ed.ptr.value, 2, cd.ptr.value, 5, float("nan"), tail=TAIL, fill=FILL),
            lambda: engine._check(L.ksp_edges_cluster_report(0, n, ed.ptr, 2, cd.ptr, 5, 0.0, pc, None, pm)),         # NULL outputs
            lambda: engine._check(L.ksp_edges_cluster_report(0, n, ed.ptr, 2, cd.ptr, 5, 0.0, None, pn, pm)),
            lambda: engine._check(L.ksp_edges_cluster_report(0, n, ed.ptr, 2, cd.ptr, 5, 0.0, pc, pn, None)),
            lambda: engine._check(L.ksp_cluster_report_valued(0, n, None, None, None, 2, pc, pn, pm)),
            lambda: engine._check(L.ksp_cluster_report_valued(0, n, None, None, None, 0, pc, None, pm)),
            lambda: engine.cluster_report_valued(3, [0, 1], [1, 3], [0.5, 0.5], tail=TAIL, fill=FILL),                # an end >= n_nodes
            lambda: engine.cluster_report_valued(3, [0, 1], [1, 2], [0.5, -0.5], tail=TAIL, fill=FILL),               # below the domain
        ]
        for i, call in enumerate(arg):
            with pytest.raises(engine.KspError) as ei:
                call()
            assert ei.value.code == engine.KSP_E_ARG, i
        for call in (lambda: engine.edges_cluster_report(n, ed.ptr.value, 0xFFFFFFFF, cd.ptr.value, 5, 0.0, tail=TAIL, fill=FILL),
                     lambda: engine._check(L.ksp_cluster_report_valued(0, n, pc, pc, pc, 0xFFFFFFFF, pc, pn, pm))):
            with pytest.raises(engine.KspError) as ei:                        # 2^32 - 1 records: refused before anything is read
                call()
            assert ei.value.code == engine.KSP_E_LIMIT and "2^32 - 1" in str(ei.value)
        assert not out_c.view(np.uint8).any() and not out_m.view(np.uint8).any() and out_n[0] == 0
        for device in (engine.device_count(), -1):
            with pytest.raises(engine.KspError) as ei:
                engine.edges_cluster_report(n, ed.ptr.value, 2, cd.ptr.value, 5, 0.0, device=device, tail=TAIL, fill=FILL)
            assert ei.value.code == engine.KSP_E_HIP and "ksp_edges_cluster_report: no such device" in str(ei.value)
            with pytest.raises(engine.KspError) as ei:
                engine.cluster_report_valued(3, [0], [1], [0.5], device=device, tail=TAIL, fill=FILL)
            assert ei.value.code == engine.KSP_E_HIP and "ksp_cluster_report_valued: no such device" in str(ei.value)
        # no record at all: every node is a singleton cluster, no kernel runs
        for got in (engine.edges_cluster_report(5, 0, 0, 0, 5, 0.0, tail=TAIL, fill=FILL), engine.cluster_report_valued(5, [], [], [], tail=TAIL, fill=FILL)):
            rs.same(got, rs.report(5, [], [], []), "empty")
            assert got[0]["size"].tolist() == [1] * 5 and got[0]["medoid"].tolist() == list(range(5)) and np.isnan(got[0]["min"]).all()
            assert engine.report_counts() == dict(kept=0, single_label_chunks=0, cluster_sets=0, node_sets=0)
        cluster, member = engine.edges_cluster_report(0, 0, 0, 0, 5, 0.0, tail=TAIL, fill=FILL)
        assert len(cluster) == 0 and len(member) == 0
    finally:
        ed.free()
        cd.free()
    _check(monkeypatch, n, e, cnt, 5, 0.0)                                    # a valid call afterwards still gives the right rows


# ---- 8. the files ----------------------------------------------------------------------------------------------------------------

def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _names(n):
    return [f"genome_{i + 1}" for i in range(n)]


def _write_names(prefix, names):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {name}\n" for i, name in enumerate(names)))


def _outputs(prefix, dist, cutoff):
    tail = rs.file_tail(dist, cutoff)
    return prefix + "_kSpider_cluster_report" + tail, prefix + "_kSpider_cluster_members" + tail


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """The 400-source index of tests/test_topk_gpu.py with a .namesMap and the TSVs of engine.pairwise."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("report")
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    (d / "full").mkdir()
    prefix = str(d / "full" / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    _write_names(prefix, _names(sk.n_sources))
    engine.pairwise(prefix, 2)
    return dict(dir=d, prefix=prefix, tsv=_read(prefix + "_kSpider_pairwise.tsv"), names=_names(sk.n_sources), n=sk.n_sources)


@pytest.mark.parametrize("cutoff", [0.0, 0.1, 0.3])
def test_report_over_the_tsv(full, cutoff):
    tsv = full["tsv"].decode()
    for dist, col in DISTS.items():
        want_report, want_members, cluster, member = rs.report_tsv(tsv, full["names"], col, cutoff, dist)
        engine.cluster_report(full["prefix"], dist, cutoff)
        out_report, out_members = _outputs(full["prefix"], dist, cutoff)
        assert _read(out_report) == want_report and _read(out_members) == want_members, (dist, cutoff)
        # line k of kspider_cluster's file holds exactly the members whose cluster is k
        engine.cluster(full["prefix"], dist, cutoff)
        lines = _read(full["prefix"] + f"_kSpider_clusters_{cutoff * 100.0!r}%.tsv").decode().split("\n")[:-1]
        assert lines == rs.cluster_file_lines(cluster, member, full["names"])
        by_number = {}
        for row in want_members.decode().split("\n")[1:-1]:
            p = row.split("\t")
            by_number.setdefault(int(p[1]), []).append(p[0])
        assert [",".join(by_number[k + 1]) for k in range(len(lines))] == lines
        os.remove(out_report)
        os.remove(out_members)
        assert 1 <= len(lines) and (cutoff > 0.0 or len(lines) < full["n"] // 2)
    assert not glob.glob(str(full["dir"] / "full" / "*.partial"))


@pytest.fixture(scope="module")
def short(oracle_lib, tmp_path_factory):
    """Per column an index whose values have at most 6 digits (tests/report_inputs.py short_index), and the two-step result."""
    d = tmp_path_factory.mktemp("report_short")
    out = {}
    for dist, col in DISTS.items():
        (d / dist).mkdir()
        prefix = str(d / dist / "ix")
        color_off, sources, weights, counts = ri.short_index(col)
        oracle_lib.write_index(prefix, color_off, sources, weights, np.arange(1, 401, dtype=np.uint32), counts)
        _write_names(prefix, _names(400))
        shutil.copytree(d / dist, d / (dist + "_two_step"))
        two = str(d / (dist + "_two_step") / "ix")
        engine.pairwise(two, 2)
        engine.cluster_report(two, dist, 0.125)
        tsv = _read(two + "_kSpider_pairwise.tsv")
        want = rs.report_tsv(tsv.decode(), _names(400), col, 0.125, dist)
        files = [_read(p) for p in _outputs(two, dist, 0.125)]
        assert files == list(want[:2]) and 20 < len(want[2]) < 350 and int(want[2]["size"].max()) > 10
        out[dist] = dict(index=d / dist, tsv=tsv, seq=_read(two + "_kSpider_seqToKmersNo.tsv"), files=files)
    out["dir"] = d
    return out


@pytest.mark.parametrize("mode", ["one", "two_workers", "device_tsv"])
def test_files_from_hbm_are_byte_equal_on_short_values(short, monkeypatch, mode):
    if mode == "two_workers":
        monkeypatch.setenv("KSPIDER_DEVICES", "0,0")
    if mode == "device_tsv":
        monkeypatch.setenv("KSPIDER_TSV", "device")
    for dist in DISTS:
        d = short["dir"] / f"fused_{dist}_{mode}"
        shutil.copytree(short[dist]["index"], d)
        fused = str(d / "ix")
        engine.pairwise_and_cluster_report(fused, 2, None if dist == "max_cont" else dist, 0.125)
        assert _read(fused + "_kSpider_pairwise.tsv") == short[dist]["tsv"] and _read(fused + "_kSpider_seqToKmersNo.tsv") == short[dist]["seq"], (dist, mode)
        assert [_read(p) for p in _outputs(fused, dist, 0.125)] == short[dist]["files"], (dist, mode)
        assert not glob.glob(str(d / "*.partial"))


@pytest.mark.parametrize("sub,cutoff", [("plain", 0.0), ("nan", 0.5)])
def test_zero_weight_colours_take_the_host_edge_path(oracle_lib, tmp_path, sub, cutoff):
    """The row 3 - 4 exists only with shared_kmers = 0 (value 0, kept at cut-off 0; "nan": NaN, source 4 counts 0 k-mers, kept at
    every cut-off): it never reaches the device, and the report is made over all kept rows on the host-edge path."""
    prefix = str(tmp_path / "z")
    zw.write(oracle_lib, prefix, sub)
    engine.pairwise(prefix, 1)
    tsv = _read(prefix + "_kSpider_pairwise.tsv")
    assert any(r[:3] == ["3", "4", "0"] for r in rs.tsv_rows(tsv.decode()))
    os.remove(prefix + "_kSpider_pairwise.tsv")
    for dist, col in DISTS.items():
        engine.pairwise_and_cluster_report(prefix, 1, dist, cutoff)
        assert _read(prefix + "_kSpider_pairwise.tsv") == tsv
        want = rs.report_tsv(tsv.decode(), _names(6), col, cutoff, dist, counts=zw.COUNTS[sub])
        outs = _outputs(prefix, dist, cutoff)
        assert [_read(p) for p in outs] == list(want[:2]), (sub, dist)
        assert want[3]["label"][3] == 2 and want[3]["degree"][2] == 1             # 3 - 4 is a cluster: the row is not missing
        for p in outs:
            os.remove(p)
        engine.cluster_report(prefix, dist, cutoff)                              # the two-step result: the same clusters and sizes
        two = rs.report_tsv(tsv.decode(), _names(6), col, cutoff, dist)
        assert [_read(p) for p in outs] == list(two[:2])
        for f in ("root", "size", "edges", "nan_edges"):
            assert (two[2][f] == want[2][f]).all()
        for p in outs:
            os.remove(p)


def test_exe_and_failing_calls_leave_nothing(full, monkeypatch):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    run = subprocess.run([EXE, prefix, "avg_cont", "0.1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    want = rs.report_tsv(full["tsv"].decode(), full["names"], 4, 0.1, "avg_cont")
    outs = _outputs(prefix, "avg_cont", 0.1)
    assert [_read(p) for p in outs] == list(want[:2])
    for p in outs:
        os.remove(p)
    before = sorted(os.listdir(d))
    for call in (lambda: engine.cluster_report(prefix, "ani", 0.1), lambda: engine.pairwise_and_cluster_report(prefix, 1, "ani", 0.1),
                 lambda: engine.cluster_report(prefix, "jaccard", 0.1), lambda: engine.pairwise_and_cluster_report(prefix, 1, "jaccard", 0.1),
                 lambda: engine.cluster_report(prefix, "max_cont", float("nan")), lambda: engine.pairwise_and_cluster_report(prefix, 1, "max_cont", float("nan")),
                 lambda: engine.cluster_report(prefix, "max_cont", 1.5), lambda: engine.cluster_report(prefix, "max_cont", -0.1),
                 lambda: engine.pairwise_and_cluster_report(prefix, 1, "max_cont", 1.5)):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    for args, code in ((["ani", "0.1"], 1), (["max_cont", "x"], 2), (["max_cont"], 2), (["max_cont", "2"], 1)):
        run = subprocess.run([EXE, prefix] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert run.returncode == code and run.stderr, args
    assert sorted(os.listdir(d)) == before
    monkeypatch.setenv("KSPIDER_DEVICE", "99")
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report(prefix, "max_cont", 0.1)
    assert ei.value.code == engine.KSP_E_HIP and "ksp_cluster_report_valued: no such device" in str(ei.value) and sorted(os.listdir(d)) == before
    monkeypatch.delenv("KSPIDER_DEVICE")
    # a row above 1: refused on the device, nothing is written
    with open(prefix + "_kSpider_pairwise.tsv", "ab") as f:
        f.write(b"1\t2\t5\t1.5\t1.5\t1.5\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report(prefix, "max_cont", 0.1)
    assert ei.value.code == engine.KSP_E_ARG and sorted(os.listdir(d)) == before
    # a malformed row: refused before any file is written
    with open(prefix + "_kSpider_pairwise.tsv", "wb") as f:
        f.write(full["tsv"] + b"1\t2\t5\tzero\tzero\tzero\n")
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report(prefix, "max_cont", 0.1)
    assert ei.value.code == engine.KSP_E_IO and "malformed" in str(ei.value) and sorted(os.listdir(d)) == before
    with open(prefix + "_kSpider_pairwise.tsv", "wb") as f:
        f.write(full["tsv"])
    # an id missing from .namesMap: the TSV path refuses the kept row that names it, the fused call the source
    _write_names(prefix, ["a", "b"])
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_report(prefix, "max_cont", 0.0)
    assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value) and sorted(os.listdir(d)) == before
    os.remove(prefix + "_kSpider_pairwise.tsv")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise_and_cluster_report(prefix, 1, "max_cont", 0.1)
    assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value) and sorted(os.listdir(d)) == before

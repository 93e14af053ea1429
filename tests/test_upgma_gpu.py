"""The average-linkage tree on the GPU against the restatement in tests/upgma_restate.py: every case compares ALL rows,
exactly.  The record counts where a ballot and a chunk begin and end; grids of 1 and 2 workgroups; the path that needs more than 150
device rounds; all-tie inputs; the round whose fold sums a run of 4; a hub of 5 000 leaves on one best[] word; ignored and refused
records; the cross product above bit 64; record orders; the hand-over to the host finish at several thresholds; real ksp_edge records
in every column; every refusal; and the file-writing calls on a 400-source index.  The output array has sentinels behind it and
d_edges is compared after every call.  The inputs come from tests/upgma_inputs.py, whose properties tests/test_upgma_cpu.py checks."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_values as xv
import repr_restate as rr
import upgma_inputs as ui
import upgma_restate as ur
from kspider_amd import engine
from oracle import ref_cluster

pytestmark = pytest.mark.gpu

C = engine.UPGMA_CHUNK_EDGES
TAIL, FILL = 5, 0xA5
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "cluster_upgma")
DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}
UNIT = 65536                                                               # the k-mer count of every node of _records


def _valued(case):
    n, a, b, v = case
    return engine.upgma_valued(n, a, b, v, tail=TAIL, fill=FILL), engine.upgma_counts()


def _records(case):
    """The case as ksp_edge records over nodes of 65 536 k-mers: every value of the case is a multiple of 2^-16, so shared / 65536 is
    that float in every column."""
    n, a, b, v = case
    shared = np.round(v.astype(np.float64) * UNIT).astype(np.uint64)
    assert (shared / UNIT == v).all()
    e = np.zeros(len(a), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = a, b, shared
    return e, np.full(n, UNIT, dtype=np.uint32)


def _edges(n, e, cnt, col=5):
    """ksp_edges_upgma over e; (rows, counts)."""
    ed = engine.DeviceBuffer.from_numpy(e) if len(e) else None
    cd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(cnt, dtype=np.uint32))
    try:
        try:
            got = engine.edges_upgma(n, ed.ptr.value if ed else 0, len(e), cd.ptr.value, col, tail=TAIL, fill=FILL)
        finally:
            if len(e):
                assert (ed.to_numpy(engine.EDGE_DTYPE, len(e)) == e).all(), "d_edges was written"
        return got, engine.upgma_counts()
    finally:
        for buf in (ed, cd):
            if buf:
                buf.free()


def _want(case):
    n, a, b, v = case
    return ur.merges(n, a, b, ur.q_of(v))


def _check(case, want=None, records=True):
    """Both entry points against the restatement; returns (the rows, the counts of the valued call)."""
    want = _want(case) if want is None else want
    got, counts = _valued(case)
    ur.same(got, want, "valued")
    assert counts["longest_run"] <= 4 and counts["device_merges"] + counts["host_merges"] == len(want), counts
    if records:
        e, cnt = _records(case)
        for col in (3, 4, 5):
            got_e, counts_e = _edges(case[0], e, cnt, col)
            ur.same(got_e, want, ("records", col))
            assert counts_e == counts
    return want, counts


# ---- 1, 2. sizes and grids -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_records", ui.RECORD_COUNTS)
def test_record_counts_around_ballots_and_chunks(monkeypatch, n_records):
    monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", "16")
    want, counts = _check(ui.sparse(300, n_records, 1))
    assert len(want) <= n_records and (n_records < 63 or len(want) > 50) and (counts["rounds"] > 0) == (counts["first_pairs"] > 16), (len(want), counts)


@pytest.mark.parametrize("cap", [1, 2])
def test_every_workgroup_loops(monkeypatch, cap):
    monkeypatch.setenv("KSP_UPGMA_MAX_WORKGROUPS", str(cap))
    monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", "0")
    case = ui.sparse(3000, 3 * C + 17, 2)
    want, counts = _check(case, records=False)
    assert counts["first_pairs"] > 2 * C and counts["host_merges"] == 0 and counts["device_merges"] == len(want) > 2000, counts


# ---- 3, 4, 5. rounds, ties, runs -------------------------------------------------------------------------------------------------

def test_a_decreasing_path_needs_more_than_150_device_rounds(monkeypatch):
    monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", "0")
    want, counts = _check(ui.path(300))
    assert len(want) == 299 and counts["rounds"] > 150 and counts["host_merges"] == 0 and counts["device_merges"] == 299 and counts["handed_over"] == 0, counts


@pytest.mark.parametrize("tail", ["0", None])
def test_all_ties_root_order_decides(monkeypatch, tail):
    if tail is not None:
        monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", tail)
    want, _ = _check(ui.path(300, equal=True))
    assert len(want) == 299 and tuple(want[0]) == (0, 1, 1 << 31, 1, 1)
    want, _ = _check(ui.clique(40))
    assert len(want) == 39 and set(want["lo"].tolist()) <= set(range(0, 40, 2)) and int(want["sum_q"][-1]) * 4 == 3 * (1 << 32) * int(want["size_lo"][-1]) * int(want["size_hi"][-1])


def test_a_fold_sums_a_run_of_exactly_four(monkeypatch):
    monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", "0")
    want, counts = _check(ui.two_pairs_all_cross(), records=False)
    assert counts["longest_run"] == 4 and counts["rounds"] == 2 and [tuple(r)[:2] for r in want] == [(0, 1), (2, 3), (0, 2)], counts
    n, a, b, v = ui.two_pairs_all_cross()
    assert int(want["sum_q"][2]) == int(ur.q_of(v)[2:].sum())


# ---- 6. contention ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("equal", [False, True])
def test_a_hub_with_5000_leaves(equal):
    want, counts = _check(ui.hub(equal=equal), records=not equal)
    assert len(want) == 5000 and (want["lo"] == 0).all() and counts["first_pairs"] == 5000
    assert counts["device_merges"] == counts["rounds"] == 5000 - engine.UPGMA_TAIL_PAIRS and counts["host_merges"] == engine.UPGMA_TAIL_PAIRS, counts
    if equal:
        assert want["hi"].tolist() == list(range(1, 5001))


# ---- 7. ignored and refused records ----------------------------------------------------------------------------------------------

def test_ignored_records():
    (n, a, b, v), part = ui.ignored_records()
    inside = (a < n) & (b < n)
    want = ur.rows_of([(3, 7, 5000 << 29, 1, 1)])
    got, _ = _valued((n, a[inside], b[inside], v[inside]))                 # a NaN, a 0, 2^-33 and self pairs take no part
    ur.same(got, want)
    # ends >= n_nodes are ignored by the record path (the valued one refuses them); NaN: 0 shared over 0 k-mers; 0: nothing shared
    cnt = np.full(n, UNIT, dtype=np.uint32)
    cnt[5] = cnt[6] = 0
    e = np.zeros(len(a), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"] = a, b
    e["shared"] = np.where(np.isnan(v) | (v < 2.0 ** -16), 0, np.round(v.astype(np.float64) * UNIT)).astype(np.uint64)
    for col in (3, 4, 5):
        got, _ = _edges(n, e, cnt, col)
        ur.same(got, want, col)
    with pytest.raises(engine.KspError) as ei:
        _valued((n, a, b, v))
    assert ei.value.code == engine.KSP_E_ARG and "out of range" in str(ei.value)


@pytest.mark.parametrize("bad", [1.0000001, float("inf")])
def test_a_value_above_one_is_refused_with_nothing_written(bad):
    n, a, b, v = ui.sparse(300, C + 1, 4)
    v = v.copy()
    v[C - 3] = bad
    assert np.float32(bad) > 1
    with pytest.raises(engine.KspError) as ei:
        _valued((n, a, b, v))                                               # (the wrapper checks every byte of the outputs)
    assert ei.value.code == engine.KSP_E_ARG
    e, cnt = _records((n, a, b, np.where(v > 1, 0.5, v).astype(np.float32)))
    if bad == float("inf"):
        cnt[e["source_1"][C - 3]] = 0                                      # a count of 0 beside shared > 0
    else:
        e["shared"][C - 3] = UNIT + 1
    pick = e["source_1"] != e["source_2"]                                  # (a self pair of a node without k-mers would be refused as well)
    with pytest.raises(engine.KspError) as ei:
        _edges(n, e[pick] if bad == float("inf") else e, cnt, 5)
    assert ei.value.code == engine.KSP_E_ARG and "above 1" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        _valued((n, a, b, np.where(v > 1, -0.25, v).astype(np.float32)))
    assert ei.value.code == engine.KSP_E_ARG


# ---- 8, 9. the hostile cross product, record orders --------------------------------------------------------------------------------

def test_the_cross_product_above_bit_64():
    case = ui.hostile_cross_product()
    want, counts = _check(case, records=False)
    assert len(want) == 4000 and tuple(want[0])[:2] == (4000, 4001) and tuple(want[-1]) == (0, 2000, 1999 << 20, 2000, 2000)
    assert int(want[0]["sum_q"]) * 4000000 >= 2 ** 64 and counts["host_merges"] > 0 and counts["device_merges"] > 0


def test_the_same_graph_under_three_record_orders_and_swapped():
    results = {name: _check(case)[0] for name, case in ui.orders(ui.sparse(400, 3000, 6)).items()}
    assert len(results) == 4 and len(results["ascending"]) > 300
    for name, rows in results.items():
        assert rows.tobytes() == results["ascending"].tobytes(), name


# ---- 10. the hand-over ------------------------------------------------------------------------------------------------------------

def test_tail_pairs_settings_give_identical_rows(monkeypatch):
    case = ui.random_graph_2000()
    want = _want(case)
    seen = {}
    for tail in ("0", "1", "7", None):
        if tail is None:
            monkeypatch.delenv("KSP_UPGMA_TAIL_PAIRS", raising=False)
        else:
            monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", tail)
        _, seen[tail] = _check(case, want, records=False)
    assert seen["0"]["host_merges"] == 0 and seen["0"]["device_merges"] == len(want) and seen["0"]["handed_over"] == 0
    assert seen["7"]["handed_over"] <= 7 and seen["1"]["handed_over"] <= 1 and seen["7"]["device_merges"] > 0 and seen["7"]["rounds"] <= seen["1"]["rounds"] <= seen["0"]["rounds"]
    assert 0 < seen[None]["handed_over"] <= engine.UPGMA_TAIL_PAIRS < seen[None]["first_pairs"] and seen[None]["device_merges"] > 0 and seen[None]["host_merges"] > 0


# ---- 11. real records ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", [3, 4, 5])
def test_real_records_equal_the_valued_call_over_exact_floats(monkeypatch, col):
    monkeypatch.setenv("KSP_UPGMA_TAIL_PAIRS", "32")
    rng = np.random.default_rng(col)
    n, m = 500, 2 * C + 100
    cnt = rng.integers(1000, 5000, n).astype(np.uint32)
    e = np.zeros(m, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"] = rng.integers(0, n, m), rng.integers(0, n, m)
    e["shared"] = rng.integers(0, np.minimum(cnt[e["source_1"]], cnt[e["source_2"]]) + 1)
    v = xv.as_f32(xv.columns(e, cnt, col))
    assert np.isfinite(v).all() and v.max() <= 1 and len(set(v.tolist())) > 1000
    got, counts = _edges(n, e, cnt, col)
    valued, _ = _valued((n, e["source_1"], e["source_2"], v))
    want = ur.merges(n, e["source_1"], e["source_2"], ur.q_of(v))
    ur.same(got, want, col)
    ur.same(valued, want, col)
    assert counts["device_merges"] > 0 and counts["host_merges"] > 0


# ---- 12. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    L = engine.lib()
    rows = np.full(24 * 8, FILL, dtype=np.uint8)
    n_rows = np.full(1, 0xA5A5A5A5, dtype=np.uint32)
    pr, pn, dummy = rows.ctypes.data, n_rows.ctypes.data, rows.ctypes.data
    for call, code in ((lambda: L.ksp_edges_upgma(0, 4, None, 5, dummy, 5, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 5, None, 5, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 5, dummy, 5, None, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 5, dummy, 5, pr, None), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 5, dummy, 2, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 5, dummy, 6, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(0, 4, dummy, 2 ** 32 - 1, dummy, 5, pr, pn), engine.KSP_E_LIMIT),   # before any device call
                       (lambda: L.ksp_upgma_valued(0, 4, dummy, dummy, dummy, 2 ** 32 - 1, pr, pn), engine.KSP_E_LIMIT),
                       (lambda: L.ksp_upgma_valued(0, 4, None, dummy, dummy, 5, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_upgma_valued(0, 4, dummy, dummy, None, 5, pr, pn), engine.KSP_E_ARG),
                       (lambda: L.ksp_edges_upgma(99, 4, dummy, 0, dummy, 5, pr, pn), engine.KSP_E_HIP)):
        assert call() == code
        assert (rows == FILL).all() and n_rows[0] == 0xA5A5A5A5
    empty = np.zeros(0, dtype=np.uint32)
    for n in (0, 1, 4):
        assert len(engine.upgma_valued(n, empty, empty, empty.astype(np.float32), tail=TAIL, fill=FILL)) == 0
        assert len(engine.edges_upgma(n, 0, 0, 0, 5, tail=TAIL, fill=FILL)) == 0
        assert engine.upgma_counts() == dict(first_pairs=0, rounds=0, device_merges=0, handed_over=0, host_merges=0, longest_run=0)
    # n_nodes 0 and 1 with records: none can take part (0: every end is out of range; 1: only self pairs are in range)
    e = np.zeros(3, dtype=engine.EDGE_DTYPE)
    e["shared"] = 5
    for n in (0, 1):
        got, _ = _edges(n, e, np.full(max(n, 1), 10, dtype=np.uint32))
        assert len(got) == 0
    assert L.ksp_upgma_valued(0, 1, dummy, dummy, dummy, 0, None, pn) == engine.KSP_OK and n_rows[0] == 0   # a NULL h_rows is fine up to one node


# ---- files -----------------------------------------------------------------------------------------------------------------------

def _names_map(prefix, n):
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write(f"{i + 1} genome_{i + 1}\n")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _build(oracle_lib, d, keys, offsets, n):
    (d / "index").mkdir()
    index = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(index, keys, offsets)
    _names_map(index, n)
    shutil.copytree(d / "index", d / "full")
    prefix = str(d / "full" / "ix")
    engine.pairwise(prefix, 2)
    tsv, seq = _read(prefix + "_kSpider_pairwise.tsv"), _read(prefix + "_kSpider_seqToKmersNo.tsv")
    rows = [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]
    return dict(dir=d, prefix=prefix, tsv=tsv, seq=seq, rows=rows, n=n, names=[f"genome_{i + 1}" for i in range(n)])


@pytest.fixture(scope="module")
def full(oracle_lib, tmp_path_factory):
    """A 400-source index (the one the tree's file test builds) and the TSVs of engine.pairwise."""
    from kspider_amd import synth
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    return _build(oracle_lib, tmp_path_factory.mktemp("upgma"), sk.keys, sk.offsets, sk.n_sources)


@pytest.fixture(scope="module")
def short_digits(oracle_lib, tmp_path_factory):
    """60 sources of exactly 32 k-mers out of a pool of 200: every containment is k / 32, at most 5 significant digits in every column."""
    rng = np.random.default_rng(32)
    sketches = [np.sort(rng.choice(200, 32, replace=False)).astype(np.uint64) + 1000 for _ in range(60)]
    offsets = np.arange(61, dtype=np.uint64) * 32
    return _build(oracle_lib, tmp_path_factory.mktemp("upgma32"), np.concatenate(sketches), offsets, 60)


def _want_from_tsv(ix, col):
    a = np.array([int(r[0]) - 1 for r in ix["rows"]])
    b = np.array([int(r[1]) - 1 for r in ix["rows"]])
    v = np.array([rr.strtof(r[col]) for r in ix["rows"]], dtype=np.float32)
    return ur.merges(ix["n"], a, b, ur.q_of(v)), v


@pytest.mark.parametrize("newick", [False, True])
def test_kspider_upgma_against_the_restated_writer(full, newick):
    for dist, col in DISTS.items():
        d = full["dir"] / f"file_{dist}_{newick}"
        shutil.copytree(full["dir"] / "full", d)
        prefix = str(d / "ix")
        before = set(os.listdir(d))
        engine.upgma(prefix, dist, newick)
        new = {f"ix_kSpider_upgma_{dist}.tsv"} | ({f"ix_kSpider_upgma_{dist}.newick"} if newick else set())
        assert set(os.listdir(d)) - before == new
        want, _ = _want_from_tsv(full, col)
        assert len(want) > full["n"] // 4
        assert _read(prefix + f"_kSpider_upgma_{dist}.tsv").decode() == ur.table_text(dist, want)
        if newick:
            assert _read(prefix + f"_kSpider_upgma_{dist}.newick").decode() == ur.newick_text(full["names"], want)


def test_cuts_of_the_upgma_table(full):
    dist, col = "max_cont", 5
    d = full["dir"] / "cuts"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    engine.upgma(prefix, dist)
    want, v = _want_from_tsv(full, col)
    assert (ur.q_of(v) >= 1).all()                                         # every row takes part: at cut-off 0 the tree spans kspider_cluster's components

    def cut(c):
        engine.cluster_from_upgma(prefix, dist, c)
        return _read(prefix + f"_kSpider_clusters_upgma_{dist}_{repr(c * 100)}%.tsv").decode()
    engine.cluster(prefix, dist, 0.0)
    assert cut(0.0) == _read(ref_cluster.output_path(prefix, 0.0)).decode()
    averages = sorted({ur.average(r) for r in want})
    above = (max(int(r["sum_q"]) // (int(r["size_lo"]) * int(r["size_hi"])) for r in want) + 1) / ur.TWO32   # the first cut-off whose q is above every average
    if above <= 1:
        assert cut(above) == "".join(n + "\n" for n in full["names"])      # above the largest average every cluster is a singleton
    for c in (averages[len(averages) // 4], averages[len(averages) // 2], averages[3 * len(averages) // 4]):
        text = cut(c)
        assert text == ur.cluster_text(full["names"], ur.cut_labels(full["n"], want, c)) and 1 < text.count("\n") < full["n"]
    assert not glob.glob(str(d / "*.partial"))


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_pairwise_and_upgma(full, short_digits, monkeypatch, devices):
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    for ix, exact in ((full, False), (short_digits, True)):
        for dist, col in DISTS.items():
            d2 = ix["dir"] / f"fused_{dist}_{devices}"
            shutil.copytree(ix["dir"] / "index", d2)
            fused = str(d2 / "ix")
            engine.pairwise_and_upgma(fused, 2, dist, True)
            assert _read(fused + "_kSpider_pairwise.tsv") == ix["tsv"] and _read(fused + "_kSpider_seqToKmersNo.tsv") == ix["seq"], (dist, devices)
            assert not glob.glob(str(d2 / "*.partial"))
            got = ur.read_table(_read(fused + f"_kSpider_upgma_{dist}.tsv").decode(), dist)
            keys = [ur.order_key(tuple(int(x) for x in r)) for r in got.tolist()]
            assert keys == sorted(keys) and len(got) > ix["n"] // 4
            if exact:                                                      # at most 6 significant digits: byte-equal to kspider_upgma over that TSV
                assert all(len(r[col].replace("0.", "").lstrip("0")) <= 6 for r in ix["rows"])
                d = ix["dir"] / f"file_{dist}_{devices}"
                shutil.copytree(ix["dir"] / "full", d)
                on_file = str(d / "ix")
                engine.upgma(on_file, dist, True)
                for ext in ("tsv", "newick"):
                    assert _read(fused + f"_kSpider_upgma_{dist}.{ext}") == _read(on_file + f"_kSpider_upgma_{dist}.{ext}"), (dist, ext)


def test_pairwise_and_upgma_with_the_device_row_text(short_digits, monkeypatch):
    monkeypatch.setenv("KSPIDER_TSV", "device")
    d2 = short_digits["dir"] / "fused_text"
    shutil.copytree(short_digits["dir"] / "index", d2)
    fused = str(d2 / "ix")
    engine.pairwise_and_upgma(fused, 2, "avg_cont", False)
    assert _read(fused + "_kSpider_pairwise.tsv") == short_digits["tsv"]
    want, _ = _want_from_tsv(short_digits, 4)
    assert _read(fused + "_kSpider_upgma_avg_cont.tsv").decode() == ur.table_text("avg_cont", want)


def test_exe_and_refusals(full):
    d = full["dir"] / "exe"
    shutil.copytree(full["dir"] / "full", d)
    prefix = str(d / "ix")
    before = sorted(os.listdir(d))
    for call in (lambda: engine.pairwise_and_upgma(prefix, 1, "ani"), lambda: engine.upgma(prefix, "ani"), lambda: engine.upgma(prefix, "jaccard"),
                 lambda: engine.pairwise_and_upgma(prefix, 1, "jaccard")):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    assert sorted(os.listdir(d)) == before
    want, _ = _want_from_tsv(full, 5)
    c1, c2 = ur.average(want[len(want) // 3]), ur.average(want[2 * len(want) // 3])
    run = subprocess.run([EXE, prefix, "max_cont", "--newick", "--cut", repr(c1), "--cut", repr(c2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr
    for c in (c1, c2):
        assert _read(prefix + f"_kSpider_clusters_upgma_max_cont_{repr(c * 100)}%.tsv").decode() == ur.cluster_text(full["names"], ur.cut_labels(full["n"], want, c))
    assert _read(prefix + "_kSpider_upgma_max_cont.newick").decode() == ur.newick_text(full["names"], want) and not glob.glob(str(d / "*.partial"))
    run = subprocess.run([EXE, prefix, "jaccard"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"jaccard" in run.stderr
    run = subprocess.run([EXE, prefix, "max_cont", "--cut", "1.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 1 and b"[0, 1]" in run.stderr
    # a namesMap that does not cover the nodes: refused like kspider_cluster, and nothing new is left behind
    for path in glob.glob(prefix + "_kSpider_upgma*") + glob.glob(prefix + "_kSpider_clusters*"):
        os.remove(path)
    with open(prefix + ".namesMap", "w") as f:
        f.write("2\n1 a\n2 b\n")
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.upgma(prefix, "max_cont", True)
    assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(d)) == before
    # a row above 1 in the TSV: the domain refusal, before any file
    shutil.copy(full["dir"] / "full" / "ix.namesMap", prefix + ".namesMap")
    lines = full["tsv"].decode().split("\n")
    p = lines[1].split("\t")
    p[5] = "1.5"
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write("\n".join([lines[0], "\t".join(p)] + lines[2:]))
    before = sorted(os.listdir(d))
    with pytest.raises(engine.KspError) as ei:
        engine.upgma(prefix, "max_cont", True)
    assert ei.value.code == engine.KSP_E_ARG and sorted(os.listdir(d)) == before

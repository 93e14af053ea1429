"""Every fused drop-in call on the seeded hostile indexes of tests/fused_inputs.py (what tests/test_fused_inputs_cpu.py shows
about them holds for the oracle alone): sparse ids against a longer .namesMap, weight-0 colours, rows that exist only with
shared_kmers = 0 on either side of a source of 0 k-mers, infinite values, the cut's `unsure` pairs — with one, two and three
workers and with postings slices.  Every expected file comes from the reference side: oracle.ref_pairwise, oracle.ref_cluster
and the restatements under tests/; nothing expected is made by the code under test.

One test is one kind of call on one index in one mode.  The "all_zero" index (no posting at all) comes last.

The "derep" kind runs kspider_pairwise_and_dereplicate and, on the oracle's own TSV, kspider_dereplicate at every threshold of
fused_inputs.derep_thresholds against tests/derep_restate.py: degree-0 sources interleaved with .namesMap rows that are no source,
infinite values as members' texts, an index without a posting; it has one mode of its own, "notail" (host-driven rounds on a grid
of one workgroup).  What the restatement shows about these indexes is in tests/test_fused_inputs_cpu.py."""
import glob
import os
import shutil

import numpy as np
import pytest

import ani_restate
import cut_restate as cr
import derep_restate as dr
import fused_inputs as fz
import repr_restate as rr
import tree_restate as tr
from kspider_amd import engine
from oracle import ref_cluster

pytestmark = pytest.mark.gpu

SCALE = 1000
MODES = {"one": {}, "two": {"KSPIDER_DEVICES": "0,0"}, "three": {"KSPIDER_DEVICES": "0,0,0"}, "slices": {"KSP_SLICES": "3"}}
DEREP_MODES = {"notail": {"KSP_DEREP_TAIL": "0", "KSP_DEREP_MAX_WORKGROUPS": "1"}}      # the "derep" kind only, "tiny" and "mixed"
KINDS = ("pairwise", "cut", "cluster", "sweep", "repr", "tree", "ani", "derep")


def _params():
    out = []
    for shape, seed in fz.CASES:                                     # ("all_zero" is the last of fused_inputs.CASES)
        full = shape in ("tiny", "mixed")
        for mode in (MODES if full else ("one", "two")):
            for kind in KINDS:
                if kind != "ani" or full:
                    out.append(pytest.param(shape, seed, mode, kind, id=f"{shape}{seed}-{mode}-{kind}"))
        for mode in (DEREP_MODES if full else ()):
            out.append(pytest.param(shape, seed, mode, "derep", id=f"{shape}{seed}-{mode}-derep"))
    return out


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _make_case(oracle_lib, d, fi, ani):
    """d/index: the index and .namesMap (with ani: .extra); d/full: the same and the reference's TSVs (with ani: its ANI column)."""
    (d / "index").mkdir(parents=True)
    index = str(d / "index" / "ix")
    fz.write(oracle_lib, index, fi)
    if ani:
        with open(index + ".extra", "w") as f:
            f.write("21\n")
    shutil.copytree(d / "index", d / "full")
    prefix = str(d / "full" / "ix")
    tsv, seq = fz.reference(oracle_lib, prefix)
    case = dict(fi=fi, dir=d, prefix=prefix, tsv=tsv, seq=seq, rows=fz.rows_of(tsv), clusters={})
    if ani:
        case["ani"] = ani_restate.estimate_ani(prefix, SCALE)
        with open(prefix + "_kSpider_pairwise.ani_col.tsv", "wb") as f:
            f.write(case["ani"])
    return case


@pytest.fixture(scope="module")
def cases(oracle_lib, tmp_path_factory):
    out = {}
    for shape, seed in fz.CASES:
        d = tmp_path_factory.mktemp(f"fused_{shape}_{seed}")
        fi = fz.make(seed, shape)
        out[shape, seed] = _make_case(oracle_lib, d / "plain", fi, ani=False)
        if shape in ("tiny", "mixed"):
            out[shape, seed, "counted"] = _make_case(oracle_lib, d / "counted", fz.with_counts(fi), ani=True)
    return out


def _want_clusters(case, dist, c):
    """(file name, bytes) of oracle.ref_cluster for the reference TSV: computed once per (distance, cut-off)."""
    if (dist, c) not in case["clusters"]:
        path = ref_cluster.write_clusters(case["prefix"], dist, c)
        case["clusters"][dist, c] = (os.path.basename(path), _read(path))
        os.remove(path)
    return case["clusters"][dist, c]


def _fresh(case, tmp_path, name="run"):
    shutil.copytree(case["dir"] / "index", tmp_path / name)
    return str(tmp_path / name / "ix")


def _check_tsvs(case, prefix, want_tsv=None):
    assert _read(prefix + "_kSpider_pairwise.tsv") == (case["tsv"] if want_tsv is None else want_tsv)
    assert _read(prefix + "_kSpider_seqToKmersNo.tsv") == case["seq"]
    assert not glob.glob(os.path.join(os.path.dirname(prefix), "*.partial"))


def _forget(prefix, *patterns):
    """No output of an earlier call of this test stands in for one the next call did not write."""
    for pat in ("_kSpider_pairwise.tsv", "_kSpider_seqToKmersNo.tsv") + patterns:
        for path in glob.glob(prefix + pat):
            os.remove(path)


def _pairwise(case, tmp_path):
    for threads in (1, 3):
        prefix = _fresh(case, tmp_path, f"t{threads}")
        engine.pairwise(prefix, threads)
        _check_tsvs(case, prefix)


def _cut(case, tmp_path):
    fi, rows, text = case["fi"], case["rows"], case["tsv"].decode()
    prefix = _fresh(case, tmp_path)
    for dist, col in fz.DISTS.items():
        for c in fz.cutoffs(rows, col, outside=False):
            _forget(prefix)
            engine.pairwise_cut(prefix, 2, dist, c)
            want = cr.cut_tsv(text, col, c).encode()
            assert want == case["tsv"] or c > 0
            _check_tsvs(case, prefix, want)
    if fi.unsure and fi.shape in ("mixed", "tiny"):
        c = fz.unsure_cut(rows)
        _forget(prefix)
        engine.pairwise_cut(prefix, 1, "min_cont", c)
        got = fz.rows_of(_read(prefix + "_kSpider_pairwise.tsv"))
        pairs = {(int(r[0]), int(r[1])) for r in got}
        assert not pairs & set(fi.unsure)                             # the dropped real row is not replaced by a NaN row
        nan_only = [r for r in rows if r[2] == "0" and "nan" in r[3]]
        assert nan_only and all(r in got for r in nan_only)


def _cluster(case, tmp_path):
    prefix = _fresh(case, tmp_path)
    for dist, col in fz.DISTS.items():
        for c in fz.cutoffs(case["rows"], col, outside=True):
            _forget(prefix, "_kSpider_clusters_*")
            engine.pairwise_and_cluster(prefix, 2, dist, c)
            _check_tsvs(case, prefix)
            name, data = _want_clusters(case, dist, c)
            assert [os.path.basename(p) for p in glob.glob(prefix + "_kSpider_clusters_*")] == [name], (dist, c)
            assert _read(os.path.join(os.path.dirname(prefix), name)) == data, (dist, c)


def _sweep(case, tmp_path):
    prefix, rows = _fresh(case, tmp_path), case["rows"]
    folder = os.path.dirname(prefix)
    for dist, col in fz.DISTS.items():
        ladder = fz.cutoffs(rows, col, outside=True)
        rng = np.random.default_rng(col)
        given = [ladder[i] for i in rng.permutation(len(ladder))]
        given.insert(int(rng.integers(0, len(given))), given[0])     # shuffled, one cut-off twice
        _forget(prefix, "_kSpider_clusters_*", "_kSpider_cluster_sweep_*")
        engine.pairwise_and_cluster_sweep(prefix, 2, dist, given)
        _check_tsvs(case, prefix)
        names, summary = set(), ["cutoff_percent\tedges\tclusters\tsingletons\tlargest"]
        # composed as tests/test_sweep_gpu.py::_check_outputs composes it; a cut-off is its product with 100 (what the rows are
        # tested against and what names the file), and a printed value and the float above it can have the same one
        for c in sorted({float(c) * 100: c for c in given}.values()):
            name, data = _want_clusters(case, dist, c)
            names.add(name)
            assert _read(os.path.join(folder, name)) == data, (dist, c)
            sizes = [l.count(b",") + 1 for l in data.split(b"\n") if l]
            edges = sum(cr.keep(r[col], c) for r in rows)
            summary.append(f"{float(c) * 100}\t{edges}\t{len(sizes)}\t{sizes.count(1)}\t{max(sizes)}")
        got = _read(prefix + f"_kSpider_cluster_sweep_{dist}.tsv").decode().split("\n")
        assert got[-1] == "" and len(got) - 1 == len(summary)
        for have, want in zip(got, summary):
            assert have == want, dist
        assert {os.path.basename(p) for p in glob.glob(prefix + "_kSpider_clusters_*")} == names


def _repr(case, tmp_path):
    prefix, text = _fresh(case, tmp_path), case["tsv"].decode()
    for dist, col in fz.DISTS.items():
        picks = fz.quartiles(case["rows"], col)
        for t in [0.20, 0.0, -1.0] + picks[len(picks) // 2:len(picks) // 2 + 1]:
            _forget(prefix, "_kSpider_repr_sketches.txt")
            engine.pairwise_and_repr(prefix, 2, dist, t)
            _check_tsvs(case, prefix)
            assert _read(prefix + "_kSpider_repr_sketches.txt") == rr.repr_sketches(text, col, t), (dist, t)


def _check_newick(prefix, dist, n):
    """tests/test_tree_gpu.py::_check_newick for a tree of several clusters: they hang under one root at height 1."""
    leaves, lengths = tr.parse_newick(_read(prefix + f"_kSpider_tree_{dist}.newick").decode())
    assert set(leaves) == {f"genome_{i + 1}" for i in range(n)}
    assert all(x >= 0 for x in lengths)
    tol = 5e-7 * n                                                   # "%.6g" per branch (heights are at most 1), at most n branches on a path
    assert all(abs(d - 1.0) <= tol for d in leaves.values()), dist


def _tree(case, tmp_path):
    fi, rows = case["fi"], case["rows"]
    prefix = _fresh(case, tmp_path)
    zero_only = {(r[0], r[1]) for r in rows if r[2] == "0"}
    for dist, col in fz.DISTS.items():
        _forget(prefix)
        engine.pairwise_and_tree(prefix, 2, dist, True)
        _check_tsvs(case, prefix)
        lines = _read(prefix + f"_kSpider_tree_{dist}.tsv").decode().split("\n")
        assert lines[0] == f"source_1\tsource_2\t{dist}\tmerged_size" and lines[-1] == ""
        got = [l.split("\t") for l in lines[1:-1]]
        keys = [tr.weight_key(r[2]) for r in got]
        assert keys == sorted(keys)
        want = tr.tree_rows(fi.NN, [(int(r[0]), int(r[1]), r[col]) for r in rows])
        assert sorted(r[2] for r in got) == sorted(t for _, _, t, _ in want), dist
        n_clusters = _want_clusters(case, dist, -1.0)[1].count(b"\n")
        assert n_clusters > 1 and len(got) == fi.NN - n_clusters
        assert all(2 <= int(r[3]) <= fi.NN for r in got)
        _check_newick(prefix, dist, fi.NN)
        for c in fz.cutoffs(rows, col, outside=True):
            engine.cluster_from_tree(prefix, dist, c)
            name, data = _want_clusters(case, dist, c)
            path = os.path.join(os.path.dirname(prefix), name)
            assert _read(path) == data, (dist, c)
            os.remove(path)
        if fi.shape == "mixed":
            assert any((r[0], r[1]) in zero_only and (r[2] == "0" or "nan" in r[2]) for r in got), dist
            assert [r[:2] for r in got].count([str(v) for v in fi.zero_bridges[1]]) == 1      # the NaN row between islands 3 and 4


def _ani(case, tmp_path, counted):
    # the index as it is holds a NaN row: refused before the TSV is written
    prefix = _fresh(case, tmp_path, "refused")
    assert any(r[2] == "0" and ("nan" in r[3] or "nan" in r[5]) for r in case["rows"])
    with open(prefix + ".extra", "w") as f:
        f.write("21\n")
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise_ani(prefix, 2, SCALE, 0.5)
    assert ei.value.code == engine.KSP_E_ARG
    assert not os.path.exists(prefix + "_kSpider_pairwise.tsv") and not os.path.exists(prefix + "_kSpider_pairwise.ani_col.tsv")
    # every source given a count
    prefix = _fresh(counted, tmp_path)
    vals = sorted(float(v) for v in counted["ani"].decode().split("\n")[1:-1])
    for c in (0.0, 1.0, vals[len(vals) // 2]):
        _forget(prefix, "_kSpider_clusters_*", "_kSpider_pairwise.ani_col.tsv")
        engine.pairwise_ani(prefix, 2, SCALE, c)
        _check_tsvs(counted, prefix)
        assert _read(prefix + "_kSpider_pairwise.ani_col.tsv") == counted["ani"]
        name, data = _want_clusters(counted, "ani", c)
        assert _read(os.path.join(os.path.dirname(prefix), name)) == data, c


def _names(n):
    return [f"genome_{i + 1}" for i in range(n)]


def _want_derep(case, dist, t, n_names=None):
    """The restatement's file for the reference TSV: computed once per (distance, threshold, rows of .namesMap)."""
    n = case["fi"].NN if n_names is None else n_names
    memo = case.setdefault("derep", {})
    if (dist, t, n) not in memo:
        memo[dist, t, n] = dr.dereplicated_tsv(case["tsv"].decode(), _names(n), fz.DISTS[dist], t, dist)
    return memo[dist, t, n]


def _derep_files(prefix):
    return sorted(os.path.basename(p) for p in glob.glob(prefix + "_kSpider_dereplicated_*"))


def _derep_table(data):
    """{id: (representative id, text, degree, rank)} of a dereplicated file whose names are genome_<id>."""
    cut = len("genome_")
    return {int(p[0][cut:]): (int(p[1][cut:]), p[2], int(p[3]), int(p[4])) for p in (l.split("\t") for l in data.decode().split("\n")[1:-1])}


def _derep(case, tmp_path):
    fi, rows = case["fi"], case["rows"]
    prefix = _fresh(case, tmp_path)
    shutil.copytree(case["dir"] / "full", tmp_path / "tsv")              # the oracle's own TSV: its shared-0, NaN and inf rows
    full_prefix = str(tmp_path / "tsv" / "ix")
    for dist, col in fz.DISTS.items():
        name = f"ix_kSpider_dereplicated_{dist}.tsv"
        for t in fz.derep_thresholds(rows, col):
            want = _want_derep(case, dist, t)
            _forget(prefix, "_kSpider_dereplicated_*")
            engine.pairwise_and_dereplicate(prefix, 2, dist, t)
            _check_tsvs(case, prefix)
            assert _derep_files(prefix) == [name], (dist, t)
            got = _read(prefix + f"_kSpider_dereplicated_{dist}.tsv")
            assert got == want, (dist, t)
            engine.dereplicate(full_prefix, dist, t)
            assert _derep_files(full_prefix) == [name], (dist, t)
            assert _read(full_prefix + f"_kSpider_dereplicated_{dist}.tsv") == want, (dist, t)
            os.remove(full_prefix + f"_kSpider_dereplicated_{dist}.tsv")
            if fi.shape == "mixed" and t in (0.0, 2.0):
                _check_mixed_rows(fi, rows, col, t, _derep_table(got))
    # out_path: the same bytes there, and no file of the default name
    (tmp_path / "elsewhere").mkdir()
    out = str(tmp_path / "elsewhere" / "mine.tsv")
    _forget(prefix, "_kSpider_dereplicated_*")
    engine.pairwise_and_dereplicate(prefix, 2, "avg_cont", 0.0, out)
    _check_tsvs(case, prefix)
    assert _read(out) == _want_derep(case, "avg_cont", 0.0) and _derep_files(prefix) == []
    assert sorted(os.listdir(tmp_path / "elsewhere")) == ["mine.tsv"]


def _check_mixed_rows(fi, rows, col, t, table):
    """Read from the written file (not from a trace): at 0.0 the planted source of the rank flip has its neighbours and a row
    of .namesMap without a source ranks among the degree-0 rows; at 2.0 the source without a count entry stands, wherever it has a
    real row among this column's infinite values, with neighbours: a representative, or a member through an "inf" text."""
    assert sorted(table) == list(range(1, fi.NN + 1))
    connected = sum(deg > 0 for _, _, deg, _ in table.values())
    if t == 0.0:
        assert table[fi.rank_flip[0]][2] >= 2                          # (an island is a triangle of real rows)
        lone = [v for v in table if v not in fi.ids]
        assert lone and all(table[v][:3] == (v, "-", 0) and table[v][3] >= connected for v in lone)
    else:
        nc, = fi.no_count
        if any(r[2] != "0" and r[col] == "inf" and str(nc) in r[:2] for r in rows):
            rep, text, deg, _ = table[nc]
            assert deg > 0 and text == ("-" if rep == nc else "inf")


@pytest.mark.parametrize("seed", [seed for shape, seed in fz.CASES if shape == "tiny"])
def test_derep_refuses_an_id_beyond_names_map(cases, tmp_path, seed):
    """.namesMap one row shorter than the largest source id.  The fused call refuses before any TSV is written; the TSV call
    refuses exactly when a passing row names the missing id and otherwise writes the restatement's file for the shorter list."""
    case = cases["tiny", seed]
    fi, rows = case["fi"], case["rows"]
    short = max(fi.ids) - 1
    prefix = _fresh(case, tmp_path)
    shutil.copytree(case["dir"] / "full", tmp_path / "tsv")
    full_prefix = str(tmp_path / "tsv" / "ix")
    for p in (prefix, full_prefix):
        with open(p + ".namesMap", "w") as f:
            f.write(f"{short}\n" + "".join(f"{i + 1} genome_{i + 1}\n" for i in range(short)))
    before = sorted(os.listdir(os.path.dirname(prefix)))
    for dist in fz.DISTS:
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_and_dereplicate(prefix, 2, dist, 0.20)
        assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(os.path.dirname(prefix))) == before
    before = sorted(os.listdir(os.path.dirname(full_prefix)))
    outcomes = set()
    for dist, col in fz.DISTS.items():
        out = full_prefix + f"_kSpider_dereplicated_{dist}.tsv"
        for t in fz.derep_thresholds(rows, col):
            names_it = fz.names_beyond(rows, col, t, short)
            outcomes.add(names_it)
            if names_it:
                with pytest.raises(engine.KspError) as ei:
                    engine.dereplicate(full_prefix, dist, t)
                assert ei.value.code == engine.KSP_E_IO and "namesMap" in str(ei.value), (dist, t)
            else:
                engine.dereplicate(full_prefix, dist, t)
                assert _read(out) == _want_derep(case, dist, t, short), (dist, t)
                os.remove(out)
            assert sorted(os.listdir(os.path.dirname(full_prefix))) == before, (dist, t)
    assert False in outcomes                  # (and True for one seed at least: tests/test_fused_inputs_cpu.py)


def test_derep_calls_in_one_sequence(cases, tmp_path, monkeypatch):
    """One "mixed" prefix, one process: the fused call, another fused kind, the fused call with two workers, the TSV call on what
    they left — every file is the one-shot expectation."""
    case = cases["mixed", 1]
    prefix = _fresh(case, tmp_path)
    folder = os.path.dirname(prefix)
    engine.pairwise_and_dereplicate(prefix, 2, "avg_cont", 0.0)
    _check_tsvs(case, prefix)
    assert _read(prefix + "_kSpider_dereplicated_avg_cont.tsv") == _want_derep(case, "avg_cont", 0.0)
    _forget(prefix)
    engine.pairwise_and_cluster(prefix, 2, "max_cont", 0.0)
    _check_tsvs(case, prefix)
    cname, cdata = _want_clusters(case, "max_cont", 0.0)
    assert _read(os.path.join(folder, cname)) == cdata
    _forget(prefix)
    monkeypatch.setenv("KSPIDER_DEVICES", "0,0")
    engine.pairwise_and_dereplicate(prefix, 2, "min_cont", 0.20)
    monkeypatch.delenv("KSPIDER_DEVICES")
    _check_tsvs(case, prefix)
    engine.dereplicate(prefix, "max_cont", 2.0)
    _check_tsvs(case, prefix)
    want = {f"ix_kSpider_dereplicated_{d}.tsv": _want_derep(case, d, t) for d, t in (("avg_cont", 0.0), ("min_cont", 0.20), ("max_cont", 2.0))}
    assert _derep_files(prefix) == sorted(want)
    for name, data in want.items():
        assert _read(os.path.join(folder, name)) == data, name
    assert _read(os.path.join(folder, cname)) == cdata and len(set(want.values())) == 3


@pytest.mark.parametrize("shape,seed,mode,kind", _params())
def test_fused_call(cases, tmp_path, monkeypatch, shape, seed, mode, kind):
    for name, value in {**MODES, **DEREP_MODES}[mode].items():
        monkeypatch.setenv(name, value)
    case = cases[shape, seed]
    if kind == "ani":
        _ani(case, tmp_path, cases[shape, seed, "counted"])
    else:
        {"pairwise": _pairwise, "cut": _cut, "cluster": _cluster, "sweep": _sweep, "repr": _repr, "tree": _tree, "derep": _derep}[kind](case, tmp_path)

"""`kSpider export --newick` on the MI355X: the library against the reference's own outputs, the device
linkage against the restatement bit for bit, an index of 2 000 sources end to end, and one C2-size run."""
import os
import re
import tempfile
import time

import numpy as np
import pytest

import export_restate as er
from kspider_amd import engine, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "export")
CASES = [(c, d) for c in sorted(os.listdir(GOLD)) for d in ("min_cont", "avg_cont", "max_cont", "ani")
         if os.path.exists(os.path.join(GOLD, c, f"ref_{d}.newick"))]
SUFFIXES = ("_pairwise.tsv", "_distmat.tsv", ".newick")


@pytest.mark.parametrize("case,dist", CASES)
def test_export_newick_equals_the_reference(case, dist, tmp_path, monkeypatch):
    ref = os.path.join(GOLD, case, f"ref_{dist}")
    prefix = os.path.join(GOLD, case, "sigs")
    engine.export(prefix, dist, True, str(tmp_path / "o"))
    for suf in SUFFIXES:
        assert open(str(tmp_path / "o") + suf, "rb").read() == open(ref + suf, "rb").read(), suf
    d = tmp_path / "default"
    d.mkdir()
    monkeypatch.chdir(d)
    engine.export(prefix, dist, True)
    names = er.default_names(prefix)
    assert sorted(os.listdir(d)) == sorted(names.values())
    for suf, name in names.items():
        assert open(name, "rb").read() == open(ref + suf, "rb").read(), suf


def _linkage_on_device(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    buf = engine.DeviceBuffer.from_numpy(M)
    try:
        return engine.single_linkage_rows(buf.ptr.value, M.shape[0])
    finally:
        buf.free()


def _six_digit(rng, n, density):
    """A symmetric matrix of cells as the export makes them: read_csv(repr(1 - float('%.6g' % c))), zero diagonal."""
    c = rng.random((n, n))
    keep = np.triu(rng.random((n, n)) < density, 1)
    texts = {}
    M = np.zeros((n, n))
    for i, j in zip(*np.nonzero(keep)):
        t = "%.6g" % c[i, j]
        if t not in texts:
            texts[t] = er.xstrtod(repr(1 - float(t)))
        M[i, j] = M[j, i] = texts[t]
    return M


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 1000, 2500])
def test_single_linkage_rows_equals_the_restatement(n):
    rng = np.random.default_rng(n)
    density = 0.02 if n > 1000 else 0.3 if n > 200 else 1.0   # (keeps the restatement's sparse column loop quick)
    mats = {"zeros": np.zeros((n, n)), "random": _six_digit(rng, n, density)}
    dup = _six_digit(rng, n, density / 2)
    if n >= 4:
        dup[n // 2] = dup[1]      # duplicated rows: exact ties between their distances
        dup[:, n // 2] = dup[:, 1]
        dup[n - 1] = dup[1]
    mats["duplicated rows"] = dup
    for what, M in mats.items():
        got = _linkage_on_device(M)
        prim = er.prim_rows(er.row_pdist(M), nearest=True)
        want = er.relabel(prim[:, :3], n)
        assert got.shape == (n - 1, 4)
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), what
        buf = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(M))
        try:
            P = engine.single_linkage_prim(buf.ptr.value, n)
        finally:
            buf.free()
        assert (P.view(np.uint64) == prim.view(np.uint64)).all(), what


def test_prim_with_d_in_global_memory(monkeypatch):
    """Above 19 456 nodes D[] lives in global memory; KSP_PRIM_LDS=0 takes that path at a testable size."""
    rng = np.random.default_rng(11)
    M = _six_digit(rng, 700, 0.4)
    M[5] = M[6]
    want = er.linkage_rows(M)
    monkeypatch.setenv("KSP_PRIM_LDS", "0")
    got = _linkage_on_device(M)
    assert (got.view(np.uint64) == want.view(np.uint64)).all()


def _index(oracle_lib, d, n, seed, **kw):
    sk = synth.generate("C2", n_sources=n, seed=seed, **kw)
    prefix = os.path.join(d, "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{n}\n" + "".join(f"{i + 1} genome_{(i * 7919) % n:05d}\n" for i in range(n)))
    engine.pairwise(prefix, 4)
    return prefix


def test_synthetic_index_end_to_end(oracle_lib, tmp_path):
    prefix = _index(oracle_lib, str(tmp_path), 2000, 2024, mean_size=300, cluster_cap=30)
    for dist in ("max_cont", "min_cont"):
        out = str(tmp_path / f"o_{dist}")
        engine.export(prefix, dist, True, out)
        want = er.export(prefix, dist, True)
        for suf in SUFFIXES:
            assert open(out + suf).read() == want[suf], (dist, suf)


def _newick_leaves_and_lengths(text):
    assert text.endswith(");") and text.startswith("(")
    depth = 0
    for ch in text:
        depth += ch == "("
        depth -= ch == ")"
        assert depth >= 0
    assert depth == 0
    leaves = re.findall(r"[(,]([^(),:]+):(-?\d+\.\d\d)", text)
    lengths = [float(x) for x in re.findall(r":(-?\d+\.\d\d)", text)]
    return [x for x, _ in leaves], lengths


def _seq_dist(M, a, b, chunk=1024):
    """sqrt of the sequential sum over the columns of (M[a] - M[b])^2, vectorised over the pairs (a[k], b[k])."""
    out = np.empty(len(a))
    for k0 in range(0, len(a), chunk):
        A, B = M[a[k0:k0 + chunk]].T.copy(), M[b[k0:k0 + chunk]].T.copy()
        s = np.zeros(A.shape[1])
        for c in range(M.shape[1]):
            t = A[c] - B[c]
            s += t * t
        out[k0:k0 + chunk] = np.sqrt(s)
    return out


def test_c2_size_export(oracle_lib, capfd):
    """C2: 10 000 sources, of which 9 984 occur in the 447 298 rows of its pairwise TSV.  The tree is well formed, every
    node is a leaf exactly once, no branch length is negative.  On the matrix as read_csv reads it back, every one of the
    N - 1 Prim edges the device finds weighs exactly the host's sequential distance of its pair, and sorting and
    relabelling those rows gives the device's linkage matrix.  The device's distance matrix (the one Prim reads) equals
    the host's sequential distance on 2 * 10^4 random pairs and on every row of k_row_dist's last 64-row tile against
    256 random rows, and Prim replayed on it gives the device's rows: the minimum was taken at every step.  The wall
    time and the phases are reported."""
    pd = pytest.importorskip("pandas")
    with tempfile.TemporaryDirectory() as d:
        prefix = _index(oracle_lib, d, 10000, None)
        out = os.path.join(d, "o")
        os.environ["KSP_EXPORT_TIMES"] = "1"
        try:
            t0 = time.perf_counter()
            engine.export(prefix, "max_cont", True, out)
            wall = time.perf_counter() - t0
        finally:
            del os.environ["KSP_EXPORT_TIMES"]
        phases = capfd.readouterr().err.strip().splitlines()[-1]
        names = [ln.split()[1] for ln in open(prefix + ".namesMap").read().splitlines()[1:]]
        n_rows = sum(1 for _ in open(prefix + "_kSpider_pairwise.tsv")) - 1
        df = pd.read_csv(out + "_distmat.tsv", sep="\t")
        nodes = list(df.columns[1:])          # the names that occur in a row (a source without edges is no node)
        assert nodes == sorted(nodes) and set(nodes) <= set(names) and len(nodes) > 9900
        M = df[nodes].to_numpy(dtype=np.float64)
        del df
        leaves, lengths = _newick_leaves_and_lengths(open(out + ".newick").read())
        assert sorted(leaves) == nodes
        assert min(lengths) >= 0
    n = M.shape[0]
    buf = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(M))
    try:
        t1 = time.perf_counter()
        Z = engine.single_linkage_rows(buf.ptr.value, n)
        t_link = time.perf_counter() - t1
        P = engine.single_linkage_prim(buf.ptr.value, n)
        S = engine.row_distances(buf.ptr.value, n)
    finally:
        buf.free()
    assert (np.diff(Z[:, 2]) >= 0).all() and Z[-1, 3] == n
    x, y, m = (P[:, c].astype(np.int64) for c in (0, 1, 3))
    assert x[0] == 0 and (x[1:] == y[:-1]).all() and len(set(y.tolist()) | {0}) == n   # Prim's walk visits every node once
    merged_at = np.empty(n, dtype=np.int64)            # step at which each node joined the tree
    merged_at[0], merged_at[y] = -1, np.arange(n - 1)
    assert (merged_at[m] < np.arange(n - 1)).all()      # m was in the tree when y joined
    got = _seq_dist(M, m, y)                            # every one of the N - 1 edge weights, exactly
    assert (got.view(np.uint64) == P[:, 2].view(np.uint64)).all()
    assert (er.relabel(P[:, :3], n).view(np.uint64) == Z.view(np.uint64)).all()
    assert (P.view(np.uint64) == er.prim_rows(S, nearest=True).view(np.uint64)).all()   # the minimum at every step
    rng = np.random.default_rng(n)
    tile = np.arange((n - 1) // 64 * 64, n)             # k_row_dist's last 64-row tile (partly filled unless 64 | n)
    a = np.concatenate([rng.integers(0, n, 20000), np.repeat(tile, 256)])
    b = np.concatenate([rng.integers(0, n, 20000), rng.integers(0, n, 256 * len(tile))])
    assert (_seq_dist(M, a, b).view(np.uint64) == S[a, b].view(np.uint64)).all()
    print(f"\nC2 export --newick, {n} nodes, {n_rows} rows: {wall:.1f} s wall ({phases}); "
          f"linkage of the read-back matrix {t_link:.2f} s; all {n - 1} Prim edge weights and steps checked")


def _overflowing():
    M = np.array([[0, 1e200, 0.5], [1e200, 0, 0], [0.5, 0, 0]])   # finite cells, (1e200)^2 = inf
    return {3: M, 2: np.array([[0, 1e200], [1e200, 0]]), 200: np.pad(M, ((0, 197), (0, 197)))}


@pytest.mark.parametrize("n", [2, 3, 200])
def test_non_finite_distances_are_refused(n):
    """scipy refuses a matrix whose row distances overflow; so do all three device entry points (before Prim runs)."""
    M = np.ascontiguousarray(_overflowing()[n])
    buf = engine.DeviceBuffer.from_numpy(M)
    try:
        for f in (engine.single_linkage_rows, engine.single_linkage_prim, engine.row_distances):
            with pytest.raises(engine.KspError) as ei:
                f(buf.ptr.value, n)
            assert ei.value.code == engine.KSP_E_ARG and "not finite" in str(ei.value)
        ok = np.ascontiguousarray(np.minimum(M, 0.5))           # the same engine afterwards: still right
        buf2 = engine.DeviceBuffer.from_numpy(ok)
        try:
            got = engine.single_linkage_rows(buf2.ptr.value, n)
        finally:
            buf2.free()
        assert (got.view(np.uint64) == er.linkage_rows(ok).view(np.uint64)).all()
    finally:
        buf.free()


def test_export_with_overflowing_distance_writes_nothing(tmp_path, monkeypatch):
    d = tmp_path / "in"
    d.mkdir()
    prefix = str(d / "ix")
    with open(prefix + ".namesMap", "w") as f:
        f.write("3\n1 a\n2 b\n3 c\n")
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n1\t1\t10\n2\t2\t10\n3\t3\t10\n")
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:   # 1 - (-1e200) = 1e200: finite, but its square is not
        f.write("source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n"
                "1\t2\t1\t0.5\t0.5\t-1e200\n1\t3\t1\t0.5\t0.5\t0.5\n")
    out = tmp_path / "out"
    out.mkdir()
    monkeypatch.chdir(out)
    with pytest.raises(engine.KspError) as ei:
        engine.export(prefix, "max_cont", True, str(out / "x"))
    assert ei.value.code == engine.KSP_E_ARG and "not finite" in str(ei.value)
    assert os.listdir(out) == []
    engine.export(prefix, "min_cont", True, str(out / "x"))   # the same index, another column: fine
    assert sorted(os.listdir(out)) == ["x.newick", "x_distmat.tsv", "x_pairwise.tsv"]

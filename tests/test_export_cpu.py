"""`kSpider export` without a GPU: the restatement against the reference's own outputs, the library's
pairwise TSV and distance matrix against the same fixtures, pandas' float parser, scipy's linkage, the no-fma
property of the distance kernel, and every refusal that happens before the device is touched."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import export_restate as er
from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "export")
CASES = [(c, d) for c in sorted(os.listdir(GOLD)) for d in ("min_cont", "avg_cont", "max_cont", "ani")
         if os.path.exists(os.path.join(GOLD, c, f"ref_{d}.newick"))]
SUFFIXES = ("_pairwise.tsv", "_distmat.tsv", ".newick")


def _ref(case, dist, suf):
    return open(os.path.join(GOLD, case, f"ref_{dist}{suf}"), "rb").read()


def test_fixture_cases_cover_the_quirks():
    assert len(CASES) == 17
    dm = _ref("quirks", "max_cont", "_distmat.tsv").decode()
    assert '"b""x"' in dm and "\t0\t" in dm and "e-08" in dm and "\t1.0\t" in dm
    assert _ref("two", "max_cont", ".newick").count(b":") == 2


@pytest.mark.parametrize("case,dist", CASES)
def test_restatement_reproduces_the_reference(case, dist):
    got = er.export(os.path.join(GOLD, case, "sigs"), dist, True)
    for suf in SUFFIXES:
        assert got[suf].encode() == _ref(case, dist, suf), suf


@pytest.mark.parametrize("case,dist", CASES)
def test_library_text_outputs_equal_the_reference(case, dist, tmp_path):
    out = str(tmp_path / "o")
    engine.export(os.path.join(GOLD, case, "sigs"), dist, False, out)
    for suf in SUFFIXES[:2]:
        assert open(out + suf, "rb").read() == _ref(case, dist, suf), suf
    assert sorted(os.listdir(tmp_path)) == ["o_distmat.tsv", "o_pairwise.tsv"]


def test_default_output_names(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert engine.lib().kspider_export(os.path.join(GOLD, "setB", "sigs").encode(), None, 0, None) == 0   # NULL: max_cont
    assert sorted(os.listdir(tmp_path)) == ["kSpider_sigs_distmat.tsv", "kSpider_sigs_pairwise.tsv"]
    assert open("kSpider_sigs_distmat.tsv", "rb").read() == _ref("setB", "max_cont", "_distmat.tsv")


def _csv_domain():
    """repr(1 - float('%.6g' % c)) for every 6-digit c in [0.1, 1), a stride through every decade down to 1e-23, and
    containments 0 and 1."""
    cs = [m / 1e6 for m in range(100000, 1000000)]
    for q in range(7, 30):
        cs += [float(f"{m}e-{q}") for m in range(100000, 1000000, 97)]
    return sorted({repr(1 - float("%.6g" % c)) for c in cs + [0.0, 1.0]})


@pytest.fixture(scope="module")
def csv_domain():
    return _csv_domain()


def test_csv_float_equals_the_restatement(csv_domain):
    f = engine.csv_float
    bad = [t for t in csv_domain if f(t) != er.xstrtod(t)]
    assert not bad, bad[:5]
    assert len(csv_domain) > 900000
    # not correctly rounded: a sizeable share of the texts parse 1 ulp away from float()
    off = sum(1 for t in csv_domain[::50] if f(t) != float(t))
    assert off > len(csv_domain[::50]) // 10
    for t in ("inf", "-inf", "0", "-0.5", "1e-05", "12345678901234567890", "1.5E+3"):
        assert f(t) == er.xstrtod(t) if t != "nan" else math.isnan(f(t))
    assert math.isnan(f("nan"))
    with pytest.raises(engine.KspError):
        f("abc")


def test_csv_float_equals_pandas(csv_domain, tmp_path):
    pd = pytest.importorskip("pandas")
    texts = csv_domain[::7]
    path = tmp_path / "col.tsv"
    path.write_text("v\n" + "\n".join(texts) + "\n")
    got = pd.read_csv(path, sep="\t")["v"].to_numpy()
    want = np.array([engine.csv_float(t) for t in texts])
    assert got.dtype == np.float64 and (got.view(np.uint64) == want.view(np.uint64)).all()


def _tie_heavy(rng, n):
    vals = np.array([0.0, 0.25, 0.5, 1 - 0.0117647, 1 - 0.333333, 0.75])
    M = rng.choice(vals, size=(n, n))
    M = np.triu(M, 1)
    M = M + M.T
    if n > 3:
        M[1] = M[0]   # duplicated rows (and columns stay as they are: linkage takes any matrix)
    return M


def test_restated_linkage_equals_scipy():
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(5)
    for trial in range(120):
        n = int(rng.integers(2, 40))
        M = _tie_heavy(rng, n) if trial % 2 else np.vectorize(lambda c: er.xstrtod(repr(1 - float("%.6g" % c))))(
            rng.random((n, n)))
        want = hier.linkage(M, "single")
        got = er.linkage_rows(M)
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), trial
    Z = er.linkage_rows(np.zeros((5, 5)))
    assert (Z[:, 2] == 0).all() and Z[-1, 3] == 5


def _llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def test_row_distance_kernel_has_no_fused_multiply_add(tmp_path):
    """hipcc contracts s + t * t into v_fma_f64 unless told not to; scipy's sum is unfused."""
    obj = os.path.join(ROOT, "kspider_amd", "lib", "export.o")
    tools = [_llvm_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    assert os.path.exists(obj) and all(tools), (obj, tools)
    objcopy, bundler, objdump = tools
    fb, co = str(tmp_path / "fb.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([objcopy, f"--dump-section=.hip_fatbin={fb}", obj])
    subprocess.check_call([bundler, "--unbundle", "--type=o", f"--input={fb}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    asm = subprocess.check_output([objdump, "-d", co], text=True)
    bodies = {}
    name = None
    for line in asm.splitlines():
        if line.endswith(">:"):
            name = line.split("<")[1][:-2]
            bodies[name] = []
        elif name:
            bodies[name].append(line)
    row = [k for k in bodies if "k_row_dist" in k]
    assert len(row) == 1
    body = "\n".join(bodies[row[0]])
    assert "v_mul_f64" in body and "v_add_f64" in body
    assert "fma" not in body and "v_mfma" not in body
    # the correctly rounded sqrt lives in its own kernel (and does use fma)
    assert any("k_dist_sqrt" in k for k in bodies)


# ---- refusals that happen before the device is touched: nothing is written ----

def _write_index(d, names, rows, kmers=True):
    prefix = os.path.join(d, "ix")
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {x}\n" for i, x in enumerate(names)))
    if kmers:
        with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
            f.write("ID\tseq\tkmers\n" + "".join(f"{i + 1}\t{i + 1}\t10\n" for i in range(len(names))))
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write(er_header() + "".join(f"{a}\t{b}\t1\t{v}\t{v}\t{v}\n" for a, b, v in rows))
    return prefix


def er_header():
    return "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n"


@pytest.mark.parametrize("what,code", [
    ("unknown distance", engine.KSP_E_ARG), ("no seqToKmersNo", engine.KSP_E_IO), ("no namesMap", engine.KSP_E_IO),
    ("ani without ani_col", engine.KSP_E_IO), ("id not in namesMap", engine.KSP_E_ARG),
    ("repeated pair", engine.KSP_E_ARG), ("self pair", engine.KSP_E_ARG), ("duplicate names", engine.KSP_E_ARG),
    ("newick no rows", engine.KSP_E_ARG),
    ("newick infinite", engine.KSP_E_ARG), ("newick over the limit", engine.KSP_E_LIMIT),
    ("malformed value", engine.KSP_E_IO)])
def test_refusals_leave_no_files(tmp_path, monkeypatch, what, code):
    d = tmp_path / "in"
    d.mkdir()
    names, rows, dist, newick = ["a", "b", "c"], [(1, 2, 0.5), (2, 3, 0.25)], "max_cont", False
    if what == "unknown distance":
        dist = "jaccard"
    elif what == "ani without ani_col":
        dist = "ani"
    elif what == "id not in namesMap":
        rows.append((1, 4, 0.5))
    elif what == "repeated pair":
        rows.append((2, 1, 0.5))
    elif what == "self pair":
        rows.append((3, 3, 1.0))
    elif what == "duplicate names":
        names = ["a", "b", "a"]
    elif what == "newick no rows":
        rows, newick = [], True
    elif what == "newick infinite":
        rows, newick = rows + [(1, 3, "-inf")], True
    elif what == "newick over the limit":
        names = [f"n{i}" for i in range(65538)]
        rows, newick = [(2 * i + 1, 2 * i + 2, 0.5) for i in range(32769)], True
    elif what == "malformed value":
        rows.append((1, 3, "x"))
    prefix = _write_index(str(d), names, rows, kmers=what != "no seqToKmersNo")
    if what == "no namesMap":
        os.remove(prefix + ".namesMap")
    before = sorted(os.listdir(d))
    out = tmp_path / "out"
    out.mkdir()
    monkeypatch.chdir(out)
    for o in (None, str(out / "x")):
        with pytest.raises(engine.KspError) as ei:
            engine.export(prefix, dist, newick, o)
        assert ei.value.code == code, str(ei.value)
        assert os.listdir(out) == [] and sorted(os.listdir(d)) == before


def test_linkage_limit_is_checked_first():
    rc = engine.lib().ksp_single_linkage_rows(0, 65537, None, None)
    assert rc == engine.KSP_E_LIMIT and b"65536" in engine.lib().ksp_last_error()
    assert engine.lib().ksp_single_linkage_rows(0, 1, None, None) == engine.KSP_E_ARG
    L, host = engine.lib(), np.zeros(4)   # ksp_row_distances: the same checks, in the same order, before any device call
    assert L.ksp_row_distances(0, 65537, None, None) == engine.KSP_E_LIMIT and b"65536" in L.ksp_last_error()
    assert L.ksp_row_distances(0, 1, host.ctypes.data, host.ctypes.data) == engine.KSP_E_ARG
    assert L.ksp_row_distances(0, 2, None, host.ctypes.data) == engine.KSP_E_ARG
    assert L.ksp_row_distances(0, 2, host.ctypes.data, None) == engine.KSP_E_ARG


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 1000, 2500])
def test_oracle_row_distances_equal_the_restatement(n, oracle_lib):
    """oracle.row_pdist (the sparse column merge the size tests use as their reference) == export_restate.row_pdist bit
    for bit, on export-like cells, duplicated rows, signed and tie-heavy values, and a leading block of a wider matrix."""
    rng = np.random.default_rng(n)
    density = min(1.0, 24 / n)    # (about 24 nonzeros per row, as in the size tests: keeps the restatement quick)
    keep = np.triu(rng.random((n, n)) < density, 1)
    M = np.zeros((n, n))
    M[keep] = [er.xstrtod(repr(1 - float("%.6g" % c))) for c in rng.random(int(keep.sum()))]
    M = M + M.T
    if n >= 4:
        M[n // 2] = M[1]
        M[:, n // 2] = M[:, 1]
    wide = np.where(rng.random((n + 3, n + 3)) < density, rng.random((n + 3, n + 3)), 0.0)
    mats = {"export-like": M, "zeros": np.zeros((n, n)), "leading block": wide[:n, :n]}
    if n <= 1000:
        mats["signed"] = np.where(rng.random((n, n)) < density, rng.normal(size=(n, n)), 0.0)
    if n <= 129:
        mats["tie-heavy"] = _tie_heavy(rng, n)
    for what, A in mats.items():
        got = oracle_lib.row_pdist(A)
        want = er.row_pdist(np.ascontiguousarray(A))
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), what


def test_iterative_newick_is_not_depth_limited():
    """A chain-shaped tree 5 000 levels deep: the reference's recursion would need a raised limit."""
    n = 5000
    M = np.zeros((n, n))
    idx = np.arange(n - 1)
    M[idx, idx + 1] = M[idx + 1, idx] = 1.0
    rows = np.array([(k, k + 1, float(k + 1)) for k in range(n - 1)])
    Z = er.relabel(rows, n)
    text = er.newick(Z, [f"s{i}" for i in range(n)])
    assert text.count("(") == n - 1 and text.endswith(");")


@pytest.mark.parametrize("id_text", ["01", "+1", "1.0"])
def test_row_ids_are_matched_as_text(tmp_path, id_text):
    """The reference looks ids up in .namesMap by their text: '01' or '+1' is not '1' (a KeyError there)."""
    prefix = _write_index(str(tmp_path), ["a", "b", "c"], [(1, 2, 0.5), (id_text, 3, 0.25)])
    with pytest.raises(engine.KspError) as ei:
        engine.export(prefix, "max_cont", False, str(tmp_path / "o"))
    assert ei.value.code == engine.KSP_E_ARG and repr(id_text)[1:-1] in str(ei.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o")]


def test_ids_need_not_be_numbers(tmp_path):
    """Any id text works when the pairwise TSV uses the same text, as in the reference; a later row of an id replaces
    its name."""
    prefix = os.path.join(str(tmp_path), "ix")
    with open(prefix + ".namesMap", "w") as f:
        f.write("4\nx7 seven\n12 twelve\nq zzz\nq queue\n")
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n1\tx7\t10\n2\t12\t10\n")
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write(er_header() + "x7\t12\t1\t0.5\t0.5\t0.5\n12\tq\t1\t0.25\t0.25\t0.25\n")
    out = str(tmp_path / "o")
    engine.export(prefix, "avg_cont", False, out)
    want = er.export(prefix, "avg_cont")
    for suf in SUFFIXES[:2]:
        assert open(out + suf).read() == want[suf]
    assert "queue" in want["_distmat.tsv"] and "zzz" not in want["_distmat.tsv"]

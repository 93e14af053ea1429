"""The device's row text without a GPU: the restatement of tests/tsv_inputs.py against a golden pairwise TSV, the
inputs of tests/test_tsv_gpu.py against what they are said to be (ties that are ties, neighbours that straddle their boundary,
rows at both length bounds), and the host side under sanitizers (`make asan`: a stand-alone program, the HIP engine stubbed out):
the integer formatter of csrc/tsv_text.h — the code the device runs — against snprintf, the piece-writing file helper, and the
refusal of an unknown KSPIDER_TSV before any file is written."""
import decimal
import os
import subprocess

import numpy as np
import pytest

import tsv_inputs as ti
from kspider_amd import engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kspider_amd", "lib", "host_asan_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "clusters", "setA")
KSP_E_ARG = 1


def test_restatement_reproduces_a_golden_pairwise_tsv():
    with open(os.path.join(GOLDEN, "sigs_kSpider_pairwise.tsv"), "rb") as f:
        golden = f.read()
    header, _, body = golden.partition(b"\n")
    assert header == b"source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment"
    seq = np.loadtxt(os.path.join(GOLDEN, "sigs_kSpider_seqToKmersNo.tsv"), dtype=np.uint64, skiprows=1)
    ids = np.sort(seq[:, 1]).astype(np.uint32)                     # dense source index = rank of the group id
    counts = np.zeros(len(ids), dtype=np.uint32)
    counts[np.searchsorted(ids, seq[:, 1])] = seq[:, 2]
    rows = np.array([line.split(b"\t")[:3] for line in body.splitlines()]).astype(np.uint64)
    e = ti.edges(np.searchsorted(ids, rows[:, 0]), np.searchsorted(ids, rows[:, 1]), rows[:, 2])
    assert len(e) > 600 and ti.rows_text(e, counts, ids) == body


def test_format_floats_is_format_float():
    v = np.concatenate([ti.ties(), ti.powers_of_two(), [0, np.inf], ti.random_floats(2000, seed=3)]).astype(np.float32)
    assert engine.format_floats(v) == [engine.format_float(float(x)) for x in v] == ti.float_texts(v)


def _digits(v):
    """(the significant digits of the float's exact value, its decimal exponent)"""
    sign, digits, exp = decimal.Decimal(float(np.float32(v))).as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:
        digits.pop()
        exp += 1
    return digits, exp + len(digits) - 1


def test_ties_are_ties_in_both_directions():
    assert len(ti.TIES["even"]) >= 1 and len(ti.TIES["up"]) >= 1
    for kind, cases in ti.TIES.items():
        for v, text in cases:
            assert float(np.float32(v)) == v                          # exactly a float32
            digits, _ = _digits(v)
            assert len(digits) == 7 and digits[6] == 5, (v, digits)   # a 5 as the seventh digit and nothing behind it
            assert (digits[5] % 2 == 0) == (kind == "even"), (v, digits)
            assert engine.format_float(v) == text
            below = decimal.Decimal(float(v)) > decimal.Decimal(text)  # the text is below the value: rounded down
            assert below == (kind == "even"), (v, text)


def test_decade_and_carry_neighbours_straddle():
    for X, (lo, hi) in ti.decade_neighbours().items():
        assert hi == np.nextafter(lo, np.float32(np.inf)) and ti.exact(lo) < ti.Fraction(10) ** X <= ti.exact(hi)
        assert _digits(lo)[1] == X - 1 and _digits(hi)[1] == X
        assert ti.LO <= lo and hi < ti.HI
    for X, (lo, hi) in ti.carry_neighbours().items():
        bound = ti.Fraction(9999995, 1000000) * ti.Fraction(10) ** (X - 1)
        assert hi == np.nextafter(lo, np.float32(np.inf)) and ti.exact(lo) < bound <= ti.exact(hi)
        assert engine.format_float(float(lo)).split("e")[0].replace(".", "").lstrip("0") == "999999", (X, lo)   # six nines, no carry yet
        assert float(engine.format_float(float(hi))) == float(f"1e{X}"), (X, hi)
    # the notation changes where %g says, and it changes at the carry: scientific below 0.0001 and from 1e+06 on
    c = {X: tuple(engine.format_float(float(v)) for v in pair) for X, pair in ti.carry_neighbours().items()}
    assert c[-4] == ("9.99999e-05", "0.0001") and c[-5] == ("9.99999e-06", "1e-05")
    assert c[6] == ("999999", "1e+06") and c[5] == ("99999.9", "100000")
    assert set(ti.NOTATION_SWITCHES) <= set(c)


def test_float_inputs_are_in_the_domain():
    for v in (ti.powers_of_two(), ti.small_multiples(), ti.quotients(64), ti.ties(), ti.random_floats(1 << 12)):
        assert len(ti.in_domain(v)) == len(v) > 0
    assert len(np.unique(ti.random_floats(1 << 12).view(np.uint32) >> 23)) == 80        # every binary exponent of the domain
    assert all(not (ti.LO <= v < ti.HI) for v in ti.REFUSED)


def test_row_lengths_are_the_bounds_of_the_header():
    counts, ids = ti.extreme_tables()
    short = ti.rows_text(ti.shortest_rows(ti.C), counts, ids).split(b"\n")[:-1]
    assert {len(r) + 1 for r in short} == {ti.ROW_MIN} == {12}
    long_ = ti.rows_text(ti.longest_only(ti.C), counts, ids).split(b"\n")[:-1]
    assert {len(r) + 1 for r in long_} == {ti.ROW_MAX} == {79} and len(long_) == ti.C
    ids10, sh, fl = long_[0].split(b"\t")[:2], long_[0].split(b"\t")[2], long_[0].split(b"\t")[3:]
    assert all(len(x) == 10 for x in ids10) and len(sh) == 20 and all(len(x) == 11 and b"e+" in x for x in fl)
    alt = ti.rows_text(ti.alternating_rows(2 * ti.C + 1), counts, ids).split(b"\n")[:-1]
    assert [len(r) + 1 for r in alt[:4]] == [12, 79, 12, 79]
    # the random rows: ids, counts and shared of every width, every column inside the domain
    counts, ids = ti.node_tables()
    e = ti.rows(1 << 12)
    assert {len(str(x)) for x in ids.tolist()} == set(range(1, 11)) and len(set(ids.tolist())) == ti.N_NODES
    assert {len(str(x)) for x in e["shared"].tolist()} == set(range(1, 13))
    import repr_restate as rr
    for col in (3, 4, 5):
        assert len(ti.in_domain(rr.column_values(e, counts, col))) == len(e)
    e, counts = ti.inf_rows()
    assert b"inf" in ti.rows_text(e, counts) and b"nan" not in ti.rows_text(e, counts)
    e, counts = ti.nan_rows()
    assert b"nan" in ti.rows_text(e, counts).split(b"\n")[2]          # (the average of 0 and 0 / 0; min and max return the 0)


# ---- the host side under sanitizers ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    return EXE


def _run(exe, *args, env=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **(env or {}))
    p = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout


def test_the_devices_formatter_agrees_with_snprintf_on_the_host(exe):
    """csrc/tsv_text.h compiled for the host: every 3001st float of the domain, s / n up to 1024, j * 2^k, both length bounds (quick
    sizes: `host_asan_check tsv_text 97 4096` is the long form; the GPU test runs all of s / n up to 4096 on the device)."""
    out = _run(exe, "tsv_text", "3001", "1024")
    lines = [l for l in out.splitlines() if l.startswith(("ok ", "FAIL "))]
    assert len(lines) == 9 and all(l.startswith("ok ") for l in lines), out


def test_piece_writer(exe, tmp_path):
    out = _run(exe, "tsv_pieces", str(tmp_path))
    lines = [l for l in out.splitlines() if l.startswith(("ok ", "FAIL "))]
    assert len(lines) == 3 and all(l.startswith("ok ") for l in lines), out
    assert os.listdir(tmp_path) == []


def test_unknown_switch_value_is_refused_before_any_file(exe, oracle_lib, tmp_path):
    sk = synth.generate("C2", n_sources=40, mean_size=60, cluster_cap=6, seed=5)
    prefix = str(tmp_path / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    before = sorted(os.listdir(tmp_path))
    out = _run(exe, "index", prefix, env={"KSPIDER_TSV": "bogus"})
    line = [l for l in out.splitlines() if l.startswith("rc ")][-1]
    assert int(line.split()[1]) == KSP_E_ARG and "KSPIDER_TSV" in line and "bogus" in line
    assert sorted(os.listdir(tmp_path)) == before
    # "host" and "" are today's path: it gets as far as the engine this build does not have (KSP_E_HIP = 2)
    for value in ("host", ""):
        out = _run(exe, "index", prefix, env={"KSPIDER_TSV": value})
        assert int([l for l in out.splitlines() if l.startswith("rc ")][-1].split()[1]) == 2

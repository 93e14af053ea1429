"""The containment cut without a GPU: the restatement (tests/cut_restate.py) on hand-written rows, the entry points of the
host-only build (no HIP engine: KSP_E_HIP, never a CPU fallback) and the refusals decided before any device call."""
import os
import re
import subprocess

import numpy as np
import pytest

import cut_restate as cr
from kspider_amd import engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n"


def test_restatement_on_hand_written_rows():
    assert cr.keep("0.8", 0.8) and not cr.keep("0.799999", 0.8) and cr.keep("0.800001", 0.8)
    assert cr.keep("nan", 0.8) and cr.keep("-nan", 0.8) and cr.keep("nan", 1.0)
    assert not cr.keep("0", 0.8) and cr.keep("0", 0.0) and cr.keep("1", 1.0)
    # x 100 on both sides, as the reference: 0.07 * 100 = 7.000000000000001 is above float("0.07") * 100 only if the text is lower
    assert cr.keep("0.07", 0.07) and not cr.keep("0.0699999", 0.07)
    rows = ["1\t2\t8\t0.5\t0.65\t0.8", "1\t3\t7\t0.5\t0.649999\t0.799999", "2\t3\t0\tnan\tnan\tnan", "2\t4\t0\t0\t0\t0"]
    tsv = HEADER + "\n".join(rows) + "\n"
    assert cr.cut_tsv(tsv, 5, 0.8) == HEADER + rows[0] + "\n" + rows[2] + "\n"
    assert cr.cut_tsv(tsv, 4, 0.65) == HEADER + rows[0] + "\n" + rows[2] + "\n"
    assert cr.cut_tsv(tsv, 3, 0.5) == HEADER + "\n".join(rows[:3]) + "\n"
    assert cr.cut_tsv(tsv, 5, 0.0) == tsv
    assert cr.cut_tsv(HEADER, 5, 0.5) == HEADER
    e = np.zeros(3, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = [0, 0, 2], [1, 2, 3], [8, 7, 0]
    assert cr.edge_mask(e, np.array([10, 10, 10, 0]), 5, 0.8).tolist() == [True, False, True]   # 0.8, 0.7, nan


def test_chunk_constant_is_mirrored():
    text = open(os.path.join(ROOT, "include", "kspider_amd.h")).read()
    assert int(re.search(r"#define KSP_CUT_CHUNK_EDGES (\d+)u", text).group(1)) == engine.CUT_CHUNK_EDGES
    assert engine.CUT_CHUNK_EDGES % 256 == 0
    import kspider_amd
    assert kspider_amd.pairwise_cut is engine.pairwise_cut and kspider_amd.edges_cut is engine.edges_cut
    assert kspider_amd.pairwise_host_cut is engine.pairwise_host_cut and kspider_amd.CUT_CHUNK_EDGES == engine.CUT_CHUNK_EDGES


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "kspider_amd", "lib", "host_asan_check")


def _rc(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
    return int([l for l in p.stdout.splitlines() if l.startswith("rc ")][-1].split()[1])


def test_host_only_build_has_the_entry_points_and_no_engine(exe, oracle_lib, tmp_path):
    sk = synth.generate("C2", n_sources=60, mean_size=80, cluster_cap=8, seed=77)
    prefix = str(tmp_path / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    assert _rc(exe, "edges_cut", "x") == engine.KSP_E_HIP
    assert _rc(exe, "host_cut", "x") == engine.KSP_E_HIP
    assert _rc(exe, "cut", prefix, "max_cont", "0.5") == engine.KSP_E_HIP     # index parsed, then: no engine in this build
    assert not os.path.exists(prefix + "_kSpider_pairwise.tsv") and not os.path.exists(prefix + "_kSpider_pairwise.tsv.partial")
    assert _rc(exe, "cut", prefix, "ani", "0.5") == engine.KSP_E_ARG
    assert _rc(exe, "cut", prefix, "max_cont", "1.5") == engine.KSP_E_ARG


def test_argument_checks_need_no_device(tmp_path):
    """Refusals that are decided before any device call; a refused call writes no file."""
    for kw in (dict(dist_col=2), dict(dist_col=6), dict(cutoff=float("nan"))):
        with pytest.raises(engine.KspError) as ei:
            engine.edges_cut(0, 0, 0, 0, **kw)
        assert ei.value.code == engine.KSP_E_ARG, kw
    with pytest.raises(engine.KspError) as ei:
        engine.edges_cut(0, 5, 0, 0)                       # NULL pointers with edges
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.edges_cut(4096, 5, 8192, 4096 + 64)         # d_out inside d_edges (never dereferenced: refused first)
    assert ei.value.code == engine.KSP_E_ARG and "overlaps" in str(ei.value)
    sk = synth.from_runs([[1, 2], [2, 3]])
    for kw in (dict(dist_col=2), dict(cutoff=float("nan"))):
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_host_cut(sk.keys, sk.offsets, **kw)
        assert ei.value.code == engine.KSP_E_ARG, kw
    with pytest.raises(ValueError):
        engine.pairwise_host_cut(sk.keys, sk.offsets, kmer_counts=np.array([1, 2, 3]))
    prefix = str(tmp_path / "nope")
    for dist, cutoff in (("ani", 0.5), ("jaccard", 0.5), ("max_cont", -0.01), ("max_cont", 1.01), ("max_cont", float("nan"))):
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_cut(prefix, 1, dist, cutoff)
        assert ei.value.code == engine.KSP_E_ARG, (dist, cutoff)
    assert not list(tmp_path.iterdir())

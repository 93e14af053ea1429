"""The pairwise TSV's row text made on the GPU against the host's: floats through engine.format_floats_device
against engine.format_float (the host's snprintf; engine.format_floats is that call on many values), rows through
engine.edges_tsv against tests/tsv_inputs.rows_text, and the drop-in calls with KSPIDER_TSV=device against the same calls
without it, file by file and byte by byte.  The device's own output is never the yardstick.  Every text buffer has sentinel
bytes behind it (engine.edges_tsv checks them, and the whole buffer after a refused call), and d_edges is compared after every
call.  tests/test_tsv_cpu.py checks the inputs' properties without a GPU."""
import filecmp
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsv_inputs as ti
import zero_weight_inputs as zw
from kspider_amd import engine

pytestmark = pytest.mark.gpu

C = ti.C
TAIL = 64
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "kspider_amd", "lib", "pairwise")


# ---- 1. floats ---------------------------------------------------------------------------------------------------------------------

def _same_floats(values):
    """One device call and one host call on the same values, compared slot by slot."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    text, length = engine.format_floats_device(v, raw=True)
    want_text, want_length = engine.format_floats(v, raw=True)
    bad = np.flatnonzero((length != want_length) | (text != want_text).any(axis=1))
    assert len(bad) == 0, [(float(v[i]), bytes(text[i, :length[i]]), bytes(want_text[i, :want_length[i]])) for i in bad[:5]]
    return len(v)


def test_float_text_is_format_float_on_a_sample():
    """The list form, against engine.format_float called value by value."""
    v = np.concatenate([ti.ties(), [0, np.inf], ti.powers_of_two(), ti.random_floats(500, seed=9)]).astype(np.float32)
    assert engine.format_floats_device(v) == [engine.format_float(float(x)) for x in v]


def test_ties_round_to_even():
    for kind, cases in ti.TIES.items():
        assert engine.format_floats_device([v for v, _ in cases]) == [t for _, t in cases], kind


def test_powers_of_two_zero_and_inf():
    assert _same_floats(np.concatenate([ti.powers_of_two(), [0.0, np.inf]])) == 82
    assert engine.format_floats_device([0.0, np.inf, 1.0, 2.0 ** -40]) == ["0", "inf", "1", "9.09495e-13"]


def test_small_multiples_of_powers_of_two():
    assert _same_floats(ti.small_multiples()) > 100000


def test_quotients_up_to_4096():
    assert _same_floats(ti.quotients()) > 5000000


def test_decades_carries_and_notation_switches():
    d, c = ti.decade_neighbours(), ti.carry_neighbours()
    v = [x for X in ti.DECADES for x in (*d[X], *c[X])]
    assert _same_floats(v) == 100
    got = dict(zip(ti.DECADES, (engine.format_floats_device(c[X]) for X in ti.DECADES)))
    assert got[-4] == ["9.99999e-05", "0.0001"] and got[-5] == ["9.99999e-06", "1e-05"]
    assert got[6] == ["999999", "1e+06"] and got[5] == ["99999.9", "100000"] and got[0] == ["0.999999", "1"]


def test_random_floats_of_the_domain():
    assert _same_floats(ti.random_floats()) == 1 << 20


@pytest.mark.parametrize("bad", range(len(ti.REFUSED)))
def test_floats_outside_the_domain_are_refused(bad):
    v = np.array([1.0, 0.5, ti.REFUSED[bad], 2.0], dtype=np.float32)
    with pytest.raises(engine.KspError) as ei:
        engine.format_floats_device(v)
    assert ei.value.code == engine.KSP_E_ARG and "ksp_debug_format_floats" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.format_floats_device(np.float32([-0.0]))
    assert ei.value.code == engine.KSP_E_ARG


# ---- 2. rows -----------------------------------------------------------------------------------------------------------------------

class _Device:
    """The records, counts and ids in device memory; d_edges is compared when the block ends."""

    def __init__(self, e, counts, ids=None):
        self.e = np.ascontiguousarray(e)
        self.ed = engine.DeviceBuffer.from_numpy(self.e) if len(e) else None
        self.cd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32))
        self.idd = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32)) if ids is not None else None
        self.n_nodes = len(counts)

    def args(self):
        return (self.n_nodes, self.ed.ptr.value if self.ed else 0, len(self.e), self.cd.ptr.value, self.idd.ptr.value if self.idd else 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            if self.ed and exc[0] is None:
                assert (self.ed.to_numpy(engine.EDGE_DTYPE, len(self.e)) == self.e).all(), "d_edges was written"
        finally:
            for buf in (self.ed, self.cd, self.idd):
                if buf:
                    buf.free()


def _check_rows(e, counts, ids=None, want=None):
    """edges_tsv over e == the restatement; the size query == the bytes written; sentinels behind the text."""
    want = ti.rows_text(e, counts, ids) if want is None else want
    with _Device(e, counts, ids) as d:
        assert engine.edges_tsv_size(*d.args()) == len(want)
        got = engine.edges_tsv(*d.args(), tail=TAIL)
        assert len(got) == len(want)
        if got != want:
            at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
            raise AssertionError(("first difference at byte", at, got[max(0, at - 60):at + 60], want[max(0, at - 60):at + 60]))
    return want


@pytest.fixture(scope="module")
def tables():
    return ti.node_tables()


@pytest.fixture(scope="module")
def big(tables):
    """2^20 seeded random rows and their text by the restatement, computed once."""
    e = ti.rows(1 << 20)
    return e, ti.rows_text(e, *tables)


def _head(text, n):
    """the first n rows of a text"""
    return b"".join(r + b"\n" for r in text.split(b"\n", n)[:n])


@pytest.mark.parametrize("n", ti.ROW_COUNTS)
def test_row_counts_around_a_wave_and_a_chunk(tables, n):
    counts, ids = tables
    want = _check_rows(ti.rows(n, seed=n + 1), counts, ids)
    assert (len(want) == 0) == (n == 0) and want.count(b"\n") == n


def test_a_chunk_of_only_longest_rows():
    """LDS staging at its capacity: 256 rows of 79 bytes; with one short row in front the chunk is staged at offset 12."""
    counts, ids = ti.extreme_tables()
    e = ti.longest_only(C)
    assert len(_check_rows(e, counts, ids)) == C * ti.ROW_MAX
    for lead in (1, 15):                                       # (15 rows of 12 bytes: 180 = 11 * 16 + 4)
        both = np.concatenate([ti.shortest_rows(lead), ti.longest_only(2 * C)])
        _check_rows(both, counts, ids)


def test_shortest_and_longest_rows_alternating():
    counts, ids = ti.extreme_tables()
    want = _check_rows(ti.alternating_rows(3 * C + 17), counts, ids)
    assert {len(r) + 1 for r in want.split(b"\n")[:-1]} == {ti.ROW_MIN, ti.ROW_MAX}
    assert len(_check_rows(ti.shortest_rows(2 * C + 5), counts, ids)) == (2 * C + 5) * ti.ROW_MIN


def test_without_an_id_table_and_with_a_permuted_one(tables):
    counts, ids = tables
    e = ti.rows(C + 9, seed=77)
    plain = _check_rows(e, counts, None)
    permuted = _check_rows(e, counts, ids)
    assert plain != permuted and plain.split(b"\n")[0].split(b"\t")[:2] == [str(int(e["source_1"][0])).encode(), str(int(e["source_2"][0])).encode()]


def test_sources_of_zero_kmers_print_inf():
    e, counts = ti.inf_rows()
    want = _check_rows(e, counts)
    assert want.startswith(b"0\t1\t4\tinf\tinf\tinf\n0\t2\t5\t1\tinf\tinf\n") and want.endswith(b"3\t4\t0\t0\t0\t0\n")


def test_a_million_random_rows(tables, big):
    e, want = big
    assert len(want) > 40 << 20
    _check_rows(e, *tables, want=want)


def test_three_workgroups_loop_over_forty_chunks(monkeypatch, tables, big):
    e, want = big
    n = 40 * C - 3
    monkeypatch.setenv("KSP_TSV_MAX_WORKGROUPS", "3")
    _check_rows(e[:n], *tables, want=_head(want, n))


def test_pieces_that_end_inside_rows(monkeypatch, tables, big):
    """KSP_TSV_PIECE = 997 bytes: about fifty pieces per window of text, every window several chunks, none ending with a row."""
    e, want = big
    n = 9 * C + 100
    head = _head(want, n)
    assert len(head) % 997 != 0 and len(head) > 100 * 997
    monkeypatch.setenv("KSP_TSV_PIECE", "997")
    _check_rows(e[:n], *tables, want=head)
    monkeypatch.setenv("KSP_TSV_PIECE", "1")                     # a piece per byte, on a few rows
    _check_rows(e[:5], *tables, want=_head(want, 5))


def test_overflow_leaves_the_buffer_untouched(tables):
    counts, ids = tables
    e = ti.rows(C + 1, seed=4)
    want = ti.rows_text(e, counts, ids)
    with _Device(e, counts, ids) as d:
        for capacity in (len(want) - 1, 0):
            with pytest.raises(engine.KspError) as ei:
                engine.edges_tsv(*d.args(), capacity=capacity, tail=TAIL)      # (edges_tsv checks that nothing was written)
            assert ei.value.code == engine.KSP_E_OVERFLOW and "ksp_edges_tsv" in str(ei.value) and str(len(want)) in str(ei.value)
        assert engine.edges_tsv(*d.args(), capacity=len(want) + 5, tail=TAIL) == want


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------

def _refused(d, code, what, capacity=4096):
    with pytest.raises(engine.KspError) as ei:
        engine.edges_tsv(*d, capacity=capacity, tail=TAIL)
    assert ei.value.code == code and what in str(ei.value), str(ei.value)


def test_refusals(tables):
    counts, ids = tables
    n = len(counts)
    e = ti.rows(C + 30, seed=8)
    for field in ("source_1", "source_2"):                         # an end = n_nodes, in the second chunk
        bad = e.copy()
        bad[field][C + 7] = n
        with _Device(bad, counts, ids) as d:
            _refused(d.args(), engine.KSP_E_ARG, "ksp_edges_tsv", capacity=100 * len(bad))
            with pytest.raises(engine.KspError):
                engine.edges_tsv_size(*d.args())
    en, cn = ti.nan_rows()                                          # a NaN column
    with _Device(en, cn) as d:
        _refused(d.args(), engine.KSP_E_ARG, "ksp_edges_tsv")
    with _Device(ti.edges([0], [1], [1 << 45]), [1, 1]) as d:      # a column of 2^45: outside the formatter's domain
        _refused(d.args(), engine.KSP_E_ARG, "ksp_edges_tsv")
    with _Device(e, counts, ids) as d:
        nn, ep, ne, cp, ip = d.args()
        _refused((nn, 0, ne, cp, ip), engine.KSP_E_ARG, "ksp_edges_tsv: NULL")          # NULL d_edges with n_edges > 0
        _refused((nn, ep, ne, 0, ip), engine.KSP_E_ARG, "ksp_edges_tsv: NULL")          # NULL d_kmer_counts
        buf = np.full(64, 0xA5, dtype=np.uint8)
        rc = engine.lib().ksp_edges_tsv(0, nn, ep, ne, cp, ip, buf.ctypes.data, 64, None)   # NULL n_bytes
        assert rc == engine.KSP_E_ARG and b"ksp_edges_tsv: NULL" in engine.lib().ksp_last_error() and (buf == 0xA5).all()
        with pytest.raises(engine.KspError) as ei:                  # a device that does not exist
            engine.edges_tsv(*d.args(), device=99, capacity=4096, tail=TAIL)
        assert ei.value.code == engine.KSP_E_HIP and "ksp_edges_tsv: no such device" in str(ei.value)
        assert engine.edges_tsv(nn, 0, 0, cp, ip, tail=TAIL) == b""  # no rows: no bytes, KSP_OK


# ---- 4. the drop-in calls ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def index(oracle_lib, tmp_path_factory):
    """The 400-source index of the other consumer tests, with a .namesMap."""
    from kspider_amd import synth
    d = tmp_path_factory.mktemp("tsv")
    sk = synth.generate("C2", n_sources=400, mean_size=300, cluster_cap=25, seed=1234)
    (d / "index").mkdir()
    prefix = str(d / "index" / "ix")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{sk.n_sources}\n" + "".join(f"{i + 1} genome_{i + 1}\n" for i in range(sk.n_sources)))
    return d


CALLS = {
    "pairwise": lambda p: engine.pairwise(p, 2),
    "pairwise_cut": lambda p: engine.pairwise_cut(p, 2, "max_cont", 0.3),
    "pairwise_and_cluster": lambda p: engine.pairwise_and_cluster(p, 2, "avg_cont", 0.25),
    "pairwise_and_topk": lambda p: engine.pairwise_and_topk(p, 2, "min_cont", 3),
    "exe": None,
}


def _verbose_line(out):
    lines = [l for l in out.splitlines() if l.startswith("kspider_amd: pairwise TSV written by")]
    assert len(lines) <= 1
    return lines[0] if lines else ""


def _run_call(name, prefix, capfd, env):
    """The call in this process (the executable: in a child), with env set for its duration; returns what it printed."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        if name == "exe":
            run = subprocess.run([EXE, prefix, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, text=True)
            assert run.returncode == 0, run.stderr
            return run.stdout
        capfd.readouterr()
        (name if callable(name) else CALLS[name])(prefix)
        return capfd.readouterr().out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _same_dirs(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and not [n for n in names if n.endswith(".partial")]
    assert any(n.endswith("_kSpider_pairwise.tsv") for n in names)
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    return names


@pytest.mark.parametrize("devices", [None, "0,0"])
@pytest.mark.parametrize("name", list(CALLS))
def test_drop_in_files_are_identical(index, capfd, name, devices):
    host, dev = index / f"host_{name}_{devices}", index / f"dev_{name}_{devices}"
    shutil.copytree(index / "index", host)
    shutil.copytree(index / "index", dev)
    env = {"KSPIDER_VERBOSE": "1", **({"KSPIDER_DEVICES": devices} if devices else {})}
    out = _run_call(name, str(host / "ix"), capfd, env)
    assert _verbose_line(out) == ""                                 # without the switch nothing is said, nothing changes
    out = _run_call(name, str(dev / "ix"), capfd, {**env, "KSPIDER_TSV": "device"})
    line = _verbose_line(out)
    assert "written by the device" in line, out
    assert ("the records stayed on the device" in line) == (name in ("pairwise", "pairwise_cut", "exe")), line
    names = _same_dirs(host, dev)
    assert os.path.getsize(dev / "ix_kSpider_pairwise.tsv") > 1000 and len(names) >= 5
    out = _run_call(name, str(host / "ix"), capfd, {**env, "KSPIDER_TSV": "host"})      # "host" is the unset path
    assert _verbose_line(out) == ""
    _same_dirs(host, dev)


@pytest.mark.parametrize("sub", ["plain", "nan"])
def test_weight_zero_colours_fall_back_to_the_host(oracle_lib, tmp_path, capfd, sub):
    for d in ("host", "dev"):
        (tmp_path / d).mkdir()
        zw.write(oracle_lib, str(tmp_path / d / "z"), sub)
    _run_call("pairwise", str(tmp_path / "host" / "z"), capfd, {})
    out = _run_call("pairwise", str(tmp_path / "dev" / "z"), capfd, {"KSPIDER_VERBOSE": "1", "KSPIDER_TSV": "device"})
    assert "written by the host (rows of weight-0 colours" in _verbose_line(out), out
    _same_dirs(tmp_path / "host", tmp_path / "dev")


def test_a_source_of_zero_kmers_falls_back_to_the_host(oracle_lib, tmp_path, capfd):
    """Colours of positive weight only, but source 2 counts 0 k-mers: its rows print inf, and the host prints them."""
    co = np.array([0, 2, 5], dtype=np.uint32)
    src = np.array([1, 2, 1, 2, 3], dtype=np.uint32)
    for d in ("host", "dev"):
        (tmp_path / d).mkdir()
        oracle_lib.write_index(str(tmp_path / d / "z"), co, src, np.array([3, 2], dtype=np.uint32), np.arange(1, 4, dtype=np.uint32), np.array([10, 0, 30]))
    _run_call("pairwise", str(tmp_path / "host" / "z"), capfd, {})
    out = _run_call("pairwise", str(tmp_path / "dev" / "z"), capfd, {"KSPIDER_VERBOSE": "1", "KSPIDER_TSV": "device"})
    assert "written by the host (a source has 0 k-mers)" in _verbose_line(out), out
    _same_dirs(tmp_path / "host", tmp_path / "dev")
    with open(tmp_path / "dev" / "z_kSpider_pairwise.tsv", "rb") as f:
        assert b"inf" in f.read()


def test_an_ani_call_falls_back_to_the_host(index, capfd):
    host, dev = index / "host_ani", index / "dev_ani"
    for d in (host, dev):
        shutil.copytree(index / "index", d)
        with open(d / "ix.extra", "w") as f:
            f.write("21\n")
    ani = lambda p: engine.pairwise_ani(p, 2, 1000)
    _run_call(ani, str(host / "ix"), capfd, {})
    out = _run_call(ani, str(dev / "ix"), capfd, {"KSPIDER_VERBOSE": "1", "KSPIDER_TSV": "device"})
    assert "written by the host (the ANI column reads the rows on the host)" in _verbose_line(out), out
    _same_dirs(host, dev)


def test_an_unknown_switch_value_is_refused_with_no_file_written(index, monkeypatch):
    d = index / "bogus"
    shutil.copytree(index / "index", d)
    before = sorted(os.listdir(d))
    monkeypatch.setenv("KSPIDER_TSV", "bogus")
    for call in (CALLS["pairwise"], CALLS["pairwise_cut"], CALLS["pairwise_and_topk"]):
        with pytest.raises(engine.KspError) as ei:
            call(str(d / "ix"))
        assert ei.value.code == engine.KSP_E_ARG and "KSPIDER_TSV" in str(ei.value)
        assert sorted(os.listdir(d)) == before
    run = subprocess.run([EXE, str(d / "ix"), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode != 0 and b"KSPIDER_TSV" in run.stderr and sorted(os.listdir(d)) == before

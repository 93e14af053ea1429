"""The database file of query mode (kspider_pack, kspider_amd/csrc/sketch_pack.cpp; the format: sketch_set.h): round trip, every
refusal of the reader on a corpus made by truncating and flipping a good file at each section boundary, a failed write, a kSize
mismatch — and the same corpus through the reader built under AddressSanitizer + UBSan as a program of its own
(`make -C kspider_amd/csrc asan-pack`, linked with the stub instead of the HIP engine)."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kspider_amd", "lib", "pack_asan_check")
HEADER = 48


def _runs(seed, n, size=40, universe=500):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(universe, size=size + i, replace=False)).astype(np.uint64) for i in range(n)]


def _write_sig(path, sigs):
    text = json.dumps([{"name": "x", "signatures": [{"ksize": k, "mins": [int(m) for m in mins], "molecule": "dna"} for k, mins in sigs]}])
    with open(path, "w") as f:
        f.write(text)


@pytest.fixture(scope="module")
def bins(oracle_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("bins")
    runs = _runs(1, 5)
    runs.append(np.zeros(0, dtype=np.uint64))   # a sketch without hashes
    for i, r in enumerate(runs):
        oracle_lib.write_bin_sketch(str(d / f"g{i:02d}.bin"), r, slot_seed=50 + i)
    (d / "notes.txt").write_text("not a sketch")
    return str(d), [f"g{i:02d}" for i in range(len(runs))], runs


@pytest.fixture(scope="module")
def good(bins, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack") / "db.kspack")
    engine.pack(bins[0], 0, out, 2)
    return out, open(out, "rb").read()


def test_round_trip_of_bin_sketches(bins, good):
    _, names, runs = bins
    got = engine.pack_read(good[0])
    assert got["ksize"] == 0 and got["names"] == names
    assert got["present"].tolist() == [1] * len(runs) and got["kmers"].tolist() == [r.size for r in runs]
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([r.size for r in runs])]).tolist()
    assert (got["keys"] == np.concatenate(runs)).all()
    assert not os.path.exists(good[0] + ".partial")


def test_round_trip_of_signatures(tmp_path):
    d = tmp_path / "sigs"
    d.mkdir()
    a, b = [9, 3, 7, 3], [2**64 - 1, 0, 5]
    _write_sig(str(d / "a.sig"), [(21, [1, 2]), (31, a)])
    _write_sig(str(d / "b.sig"), [(21, [4, 5, 6])])             # no signature of ksize 31: a name without a sketch
    with gzip.open(str(d / "c.sig"), "wt") as f:                  # gzip content under a .sig name is read
        f.write(json.dumps([{"signatures": [{"ksize": 31, "mins": b}]}]))
    (d / "d.gz").write_bytes(b"")                                 # a bare .gz name: a group, never read
    out = str(tmp_path / "s.kspack")
    engine.pack(str(d), 31, out, 3)
    got = engine.pack_read(out)
    assert got["ksize"] == 31 and got["names"] == ["a", "b", "c", "d"]
    assert got["present"].tolist() == [1, 0, 1, 0]
    assert got["kmers"].tolist() == [4, 0, 3, 0]                  # the count of mins, duplicates included, as the reference stores it
    assert got["offsets"].tolist() == [0, 3, 6] and got["keys"].tolist() == [3, 7, 9, 0, 5, 2**64 - 1]


def _sections(blob):
    """Byte offsets where the sections of a pack file begin, and its end."""
    version, ksize, G, S, K, B = struct.unpack_from("<IiQQQQ", blob, 8)
    pad = lambda n: (n + 7) & ~7
    at = [0, HEADER]
    for size in (pad(4 * G), pad(G), 8 * (S + 1), 8, 8 * (G + 1), pad(B), 8 * K):
        at.append(at[-1] + size)
    assert at[-1] == len(blob)
    return dict(zip(("magic", "kmers", "present", "offsets", "name_count", "name_offsets", "text", "keys", "end"), at)), (G, S, K, B)


def _corpus(blob):
    """(name, bytes) of files the reader must refuse."""
    at, (G, S, K, B) = _sections(blob)
    u64 = lambda v: struct.pack("<Q", v)
    put = lambda pos, b: blob[:pos] + b + blob[pos + len(b):]
    out = [("empty", b""), ("header_only", blob[:HEADER]), ("one_byte_more", blob + b"\0"), ("eight_bytes_more", blob + bytes(8))]
    for name, pos in at.items():                                   # cut at and just before every section boundary
        if name != "end":
            out.append((f"cut_at_{name}", blob[:pos]))
        if pos:
            out.append((f"cut_before_{name}", blob[:pos - 1]))
    out.append(("magic", put(0, b"X")))
    out.append(("magic_last_byte", put(7, b"2")))
    out.append(("version", put(8, struct.pack("<I", 2))))
    for i, field in enumerate(("groups", "with_sketch", "keys", "name_bytes")):
        old = struct.unpack_from("<Q", blob, 16 + 8 * i)[0]
        out.append((f"{field}_plus_1", put(16 + 8 * i, u64(old + 1))))
        out.append((f"{field}_minus_1", put(16 + 8 * i, u64(old - 1))))
        out.append((f"{field}_huge", put(16 + 8 * i, u64(2**63 + 5))))
    out.append(("presence_cleared", put(at["present"], b"\0")))    # the count of present groups disagrees with the header
    out.append(("presence_2", put(at["present"], b"\2")))
    out.append(("offsets_start_at_1", put(at["offsets"], u64(1))))
    first = struct.unpack_from("<Q", blob, at["offsets"] + 8)[0]
    out.append(("offsets_decrease", put(at["offsets"] + 16, u64(first - 1))))
    out.append(("offsets_end_elsewhere", put(at["offsets"] + 8 * S, u64(K - 1))))
    out.append(("name_count", put(at["name_count"], u64(G + 1))))
    out.append(("name_offsets_start_at_1", put(at["name_offsets"], u64(1))))
    out.append(("name_offsets_decrease", put(at["name_offsets"] + 8, u64(B + 1))))
    out.append(("name_offsets_end_elsewhere", put(at["name_offsets"] + 8 * G, u64(B - 1))))
    k0, k1 = struct.unpack_from("<QQ", blob, at["keys"])
    out.append(("run_descends", put(at["keys"], u64(k1) + u64(k0))))
    out.append(("run_repeats", put(at["keys"] + 8, u64(k0))))
    last = at["keys"] + 8 * (first - 1)                            # the last key of the first run may exceed the next run's first
    out.append(("run_end_descends", put(last, u64(0))))
    return out


@pytest.fixture(scope="module")
def corpus(good, tmp_path_factory):
    d = tmp_path_factory.mktemp("corpus")
    files = []
    for name, blob in _corpus(good[1]):
        path = str(d / (name + ".kspack"))
        with open(path, "wb") as f:
            f.write(blob)
        files.append(path)
    return files


def test_reader_refuses_every_damaged_file(good, corpus):
    assert len(corpus) > 40
    for path in corpus:
        with pytest.raises(engine.KspError) as ei:
            engine.pack_read(path)
        assert ei.value.code == engine.KSP_E_IO, path
        assert os.path.basename(path) in str(ei.value)               # the message names the file
    with pytest.raises(engine.KspError) as ei:
        engine.pack_read(good[0] + ".missing")
    assert ei.value.code == engine.KSP_E_IO
    engine.pack_read(good[0])                                        # and the good file is still read


def test_refusal_messages_name_the_fault(good, corpus):
    by_name = {os.path.basename(p)[:-7]: p for p in corpus}
    for name, text in [("magic", "magic"), ("version", "version"), ("one_byte_more", "header implies"), ("cut_at_keys", "header implies"),
                       ("offsets_start_at_1", "do not start at 0"), ("offsets_decrease", "decrease"), ("run_repeats", "strictly ascending"),
                       ("run_descends", "strictly ascending"), ("name_count", "name count"), ("presence_cleared", "marked")]:
        with pytest.raises(engine.KspError) as ei:
            engine.pack_read(by_name[name])
        assert text in str(ei.value), (name, str(ei.value))


def test_failed_write_leaves_no_file(bins, tmp_path):
    missing = str(tmp_path / "no_such_dir" / "db.kspack")
    with pytest.raises(engine.KspError) as ei:
        engine.pack(bins[0], 0, missing, 1)
    assert ei.value.code == engine.KSP_E_IO and not os.path.exists(os.path.dirname(missing))
    taken = tmp_path / "taken.kspack"                                # the final name is a directory that is not empty: the rename fails
    taken.mkdir()
    (taken / "x").write_text("x")
    with pytest.raises(engine.KspError) as ei:
        engine.pack(bins[0], 0, str(taken), 1)
    assert ei.value.code == engine.KSP_E_IO
    assert sorted(os.listdir(tmp_path)) == ["taken.kspack"] and os.listdir(taken) == ["x"]
    with pytest.raises(engine.KspError) as ei:                       # nothing to pack: no file either
        engine.pack(str(taken), 0, str(tmp_path / "empty.kspack"), 1)
    assert ei.value.code == engine.KSP_E_IO and sorted(os.listdir(tmp_path)) == ["taken.kspack"]
    for args in [(None, 0, str(tmp_path / "o"), 1), (bins[0], -1, str(tmp_path / "o"), 1)]:
        with pytest.raises((engine.KspError, TypeError)):
            engine.pack(*args)


def test_ksize_mismatch_is_an_argument_error(bins, good, tmp_path):
    out = str(tmp_path / "out")
    with pytest.raises(engine.KspError) as ei:
        engine.query(good[0], bins[0], 31, out, 1)                   # the pack was made with kSize 0
    assert ei.value.code == engine.KSP_E_ARG and "kSize" in str(ei.value)
    for args in [(good[0], bins[0], 0, "", 1), (good[0], bins[0], -3, out, 1)]:
        with pytest.raises(engine.KspError) as ei:
            engine.query(*args)
        assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.query(good[0], bins[0], 0, out, 1, mode=5)
    assert ei.value.code == engine.KSP_E_ARG
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]


def test_corpus_under_the_sanitizers(good, corpus, bins, tmp_path):
    """The stand-alone program reads the same corpus: the same verdict per file, and no sanitizer report."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan-pack"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=4096",
               UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        p = subprocess.run([EXE, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()

    lines = run("read", good[0], *corpus)
    assert len(lines) == 1 + len(corpus)
    assert lines[0].split()[0] == "0"
    for path, line in zip(corpus, lines[1:]):
        assert line.split(" ", 1) == [str(engine.KSP_E_IO), path]
    repacked = str(tmp_path / "again.kspack")
    assert run("pack", bins[0], "0", repacked)[-1].split()[:2] == ["rc", "0"]
    assert open(repacked, "rb").read() == good[1]                    # the same bytes as the library wrote
    # the file entry up to the device call: both sides load, then the stub's engine refuses
    assert run("query", good[0], bins[0], "0", str(tmp_path / "q"))[-1].split()[:2] == ["rc", str(engine.KSP_E_HIP)]
    assert run("query", good[0], bins[0], "31", str(tmp_path / "q"))[-1].split()[:2] == ["rc", str(engine.KSP_E_ARG)]
    assert sorted(os.listdir(tmp_path)) == ["again.kspack"]

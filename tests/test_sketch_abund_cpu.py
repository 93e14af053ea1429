"""Counted sketches without a GPU: ksp_sketch_cpu_abund against the restatement (tests/sketch_abund_restate.py), the file driver
in host mode with KSP_SKETCH_ABUND (the bytes, the batches, counts that add over the pieces of a cut record), ksp_sig_read, and
the same code under AddressSanitizer + UBSan as a program of its own (`make -C kspider_amd/csrc asan-sketch`)."""
import ctypes
import gzip
import hashlib
import json
import os
import random
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import sketch_abund_restate as A
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kspider_amd", "lib", "sketch_asan_check")
FULL = 2**64 - 1


def _cases(k):
    return [I.mixed(), A.homopolymer(k), A.mirror(k), A.abutting(k), A.repeat_over_tile_edge(k)] + list(A.reads())


@pytest.mark.parametrize("k", [1, 21, 31, 33, 64])
def test_cpu_loop_against_the_restatement(k):
    for case in _cases(k):
        for mh in (FULL, R.max_hash_of(3)):
            keys, abund, off = engine.sketch_cpu_abund(case.seq, case.offsets, k, max_hash=mh)
            want_keys, want_abund, want_off = A.flat(A.sketch(case.seq, case.offsets, k, mh))
            assert (off == want_off).all() and (keys == want_keys).all() and (abund == want_abund).all(), (case.name, k)
            plain, plain_off = engine.sketch_cpu(case.seq, case.offsets, k, max_hash=mh)      # the keys are the unweighted call's
            assert (plain == keys).all() and (plain_off == off).all()


def test_the_cases_hold_what_they_are_named_for():
    k = 21
    (run,) = A.sketch(A.homopolymer(k).seq, [0, 300], k, FULL)
    assert run == [(R.kmer_hash("A" * k), 300 - k + 1)]
    (run,) = A.sketch(A.mirror(k).seq, A.mirror(k).offsets, k, FULL)
    assert len(run) == 1 and run[0][1] == 3
    c = A.abutting(k)
    first, second = A.sketch(c.seq, c.offsets, k, FULL)
    shared = R.kmer_hash(c.seq[:k].decode())
    assert dict(first)[shared] == 2 and dict(second)[shared] == 1
    one = A.sketch(c.seq, [0, len(c.seq)], k, FULL)[0]
    assert sum(n for _, n in one) == sum(n for _, n in first) + sum(n for _, n in second) + (k - 1)   # the windows over the boundary
    c = A.repeat_over_tile_edge(k)
    (run,) = A.sketch(c.seq, c.offsets, k, FULL)
    left = Counter(R.source_hashes(c.seq[:I.TILE + k - 1], k))
    heavy = [h for h, n in run if n > 20]
    assert len(heavy) == 7 and all(0 < left[h] < dict(run)[h] for h in heavy)      # every heavy hash on both sides of the tile edge
    one, three = A.reads()
    (run,) = A.sketch(one.seq, one.offsets, k, FULL)
    assert len({n for _, n in run}) > 15 and max(n for _, n in run) > 25
    assert sum(n for r in A.sketch(three.seq, three.offsets, k, FULL) for _, n in r) < sum(n for _, n in run)


def test_overflow_size_query_and_refusals():
    c = I.mixed()
    lib = engine.lib()
    buf, off = np.frombuffer(c.seq, dtype=np.uint8), np.array(c.offsets, dtype=np.uint64)
    want_keys, want_abund, want_off = A.flat(A.sketch(c.seq, c.offsets, 21, FULL))
    out_off, needed = np.zeros(4, dtype=np.uint64), ctypes.c_uint64(0)
    call = lambda keys, abund, cap: lib.ksp_sketch_cpu_abund(buf.ctypes.data, buf.size, off.ctypes.data, 3, 21, FULL, 42, keys, abund, cap, out_off.ctypes.data,   # noqa: E731
                                                             ctypes.byref(needed))
    assert call(None, None, 0) == engine.KSP_E_OVERFLOW and needed.value == want_keys.size and (out_off == want_off).all()
    keys, abund = np.full(want_keys.size + 2, 7, dtype=np.uint64), np.full(want_keys.size + 2, 7, dtype=np.uint32)
    assert call(keys.ctypes.data, abund.ctypes.data, want_keys.size - 1) == engine.KSP_E_OVERFLOW and (keys == 7).all() and (abund == 7).all()
    assert call(keys.ctypes.data, abund.ctypes.data, want_keys.size) == engine.KSP_OK
    assert (keys[:-2] == want_keys).all() and (abund[:-2] == want_abund).all() and (keys[-2:] == 7).all() and (abund[-2:] == 7).all()
    assert call(keys.ctypes.data, None, 5) == engine.KSP_E_ARG and call(None, abund.ctypes.data, 5) == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_cpu_abund(c.seq, c.offsets, 65, max_hash=FULL)
    assert ei.value.code == engine.KSP_E_ARG


# ---- the file driver in host mode

K, SCALED = 21, 2


def _fasta(records):
    return "".join(">" + name + "\n" + "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n" for name, seq in records)


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """A directory of three inputs and the bytes the reader hands on for each: reads at three depths (FASTQ-free: FASTA records of
    80 bases), one record of 6 000 bases whose middle is a tandem repeat — a small batch cuts through the repeat —, and an empty
    file."""
    d = tmp_path_factory.mktemp("samples")
    rng = random.Random(51)
    one, _ = A.reads()
    reads = [(f"r{i}", s) for i, s in enumerate(one.seq.decode().split("\n")) if s]
    unit = I.bases(rng, 5)
    long_rec = I.bases(rng, 1500) + unit * 600 + I.bases(rng, 1500)
    sources = {"reads": reads, "repeat": [("chr", long_rec), ("tail", I.bases(rng, 300))], "void": []}
    for name, recs in sources.items():
        (d / (name + ".fa")).write_text(_fasta(recs))
    return str(d), {name: "".join(seq + "\n" for _, seq in recs).encode() for name, recs in sources.items()}


def _sketch_dir(monkeypatch, src, out, abund, batch_bytes=None, threads=2):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    if batch_bytes:
        monkeypatch.setenv("KSPIDER_SKETCH_BATCH_BYTES", str(batch_bytes))
    else:
        monkeypatch.delenv("KSPIDER_SKETCH_BATCH_BYTES", raising=False)
    engine.sketch_files(src, K, SCALED, str(out), threads, abund=abund)
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


def _sig_text(filename, mins, abunds=None):
    """The signature file, byte for byte, as the driver has written it since it exists; abunds: the new field behind the mins"""
    md5 = hashlib.md5((str(K) + "".join(str(m) for m in mins)).encode()).hexdigest()
    tail = "" if abunds is None else ',"abundances":[' + ",".join(str(a) for a in abunds) + "]"
    return ('[{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":"' + filename + '","license":"CC0","version":0.4,"signatures":[{"num":0,"ksize":'
            + str(K) + ',"seed":42,"max_hash":' + str(R.max_hash_of(SCALED)) + ',"molecule":"DNA","md5sum":"' + md5 + '","mins":[' + ",".join(str(m) for m in mins) + "]" + tail
            + "}]}]\n").encode()


def test_driver_writes_abundances_and_leaves_plain_files_alone(monkeypatch, samples, tmp_path):
    src, seqs = samples
    counted = _sketch_dir(monkeypatch, src, tmp_path / "counted", True)
    plain = _sketch_dir(monkeypatch, src, tmp_path / "plain", False)
    assert sorted(counted) == sorted(plain) == sorted(n + ".sig" for n in seqs)
    for name, seq in seqs.items():
        (run,) = A.sketch(seq, [0, len(seq)], K, R.max_hash_of(SCALED))
        mins, abunds = [h for h, _ in run], [n for _, n in run]
        assert plain[name + ".sig"] == _sig_text(name + ".fa", mins), name
        assert counted[name + ".sig"] == _sig_text(name + ".fa", mins, abunds), name
        sig = json.loads(counted[name + ".sig"])[0]["signatures"][0]
        assert list(sig)[-2:] == ["mins", "abundances"] and sig["abundances"] == abunds
        assert re.sub(rb',"abundances":\[[0-9,]*\]', b"", counted[name + ".sig"]) == plain[name + ".sig"]
    (run,) = A.sketch(seqs["repeat"], [0, len(seqs["repeat"])], K, R.max_hash_of(SCALED))
    assert max(n for _, n in run) >= 590 and json.loads(counted["void.sig"])[0]["signatures"][0]["abundances"] == []


def test_small_batches_give_the_same_bytes(monkeypatch, samples, tmp_path):
    """1 KiB and 4 KiB batches: sources span batches, the record of 6 000 bases is cut inside its repeat, and the counts of the
    pieces add up — a plain union would keep one piece's count."""
    src, _ = samples
    whole = _sketch_dir(monkeypatch, src, tmp_path / "whole", True)
    for i, (batch, threads) in enumerate([(4096, 2), (1024, 1), (1500, 3)]):
        assert _sketch_dir(monkeypatch, src, tmp_path / f"small{i}", True, batch, threads) == whole, batch
    assert _sketch_dir(monkeypatch, src, tmp_path / "plain_small", False, 1024) == _sketch_dir(monkeypatch, src, tmp_path / "plain_whole", False)


# ---- ksp_sig_read

def _write_sig(path, sigs, gz=False):
    text = json.dumps([{"class": "sourmash_signature", "signatures": sigs}]).encode()
    path.write_bytes(gzip.compress(text) if gz else text)
    return str(path)


def test_sig_read(tmp_path):
    p = _write_sig(tmp_path / "a.sig", [{"ksize": 31, "mins": [1], "abundances": [9]}, {"ksize": 21, "mins": [50, 7, 2**64 - 1, 7, 20, 7], "abundances": [5, 1, 0, 2, 2**32 - 1, 4]}])
    mins, abunds = engine.sig_read(p, 21)
    assert mins.tolist() == [7, 20, 50, 2**64 - 1] and abunds.tolist() == [7, 2**32 - 1, 5, 0]        # unsorted mins; a hash listed three times is summed
    mins, abunds = engine.sig_read(p, 31)
    assert mins.tolist() == [1] and abunds.tolist() == [9]
    p = _write_sig(tmp_path / "clamp.sig", [{"ksize": 21, "abundances": [2**32 - 2, 3, 2**40], "mins": [5, 5, 6]}])                # the field before the mins; sums clamp
    mins, abunds = engine.sig_read(p, 21)
    assert mins.tolist() == [5, 6] and abunds.tolist() == [2**32 - 1, 2**32 - 1]
    p = _write_sig(tmp_path / "plain.sig", [{"ksize": 21, "mins": [3, 1, 3]}])
    mins, abunds = engine.sig_read(p, 21)
    assert mins.tolist() == [1, 3] and abunds is None
    p = _write_sig(tmp_path / "z.sig.gz", [{"ksize": 21, "mins": [4, 2], "abundances": [40, 20]}], gz=True)
    mins, abunds = engine.sig_read(p, 21)
    assert mins.tolist() == [2, 4] and abunds.tolist() == [20, 40]
    p = _write_sig(tmp_path / "none.sig", [{"ksize": 21, "mins": [], "abundances": []}])
    mins, abunds = engine.sig_read(p, 21)
    assert mins.size == 0 and abunds is not None and abunds.size == 0
    for name, sigs, what in (("short.sig", [{"ksize": 21, "mins": [1, 2, 3], "abundances": [1, 2]}], "2 abundances for 3 mins"),
                             ("long.sig", [{"ksize": 21, "mins": [1], "abundances": [1, 2]}], "2 abundances for 1 mins"),
                             ("other_k.sig", [{"ksize": 31, "mins": [1], "abundances": [1]}], "ksize 21")):
        with pytest.raises(engine.KspError) as ei:
            engine.sig_read(_write_sig(tmp_path / name, sigs), 21)
        assert ei.value.code == engine.KSP_E_IO and name in str(ei.value) and what in str(ei.value), str(ei.value)
    (tmp_path / "cut.sig").write_text('[{"signatures":[{"ksize":21,"mins":[1,2],"abundances":[1,')
    for bad in ("cut.sig", "missing.sig"):
        with pytest.raises(engine.KspError) as ei:
            engine.sig_read(str(tmp_path / bad), 21)
        assert ei.value.code == engine.KSP_E_IO and bad in str(ei.value)
    # the size query and the overflow
    n, has = ctypes.c_uint64(0), ctypes.c_int(0)
    p = str(tmp_path / "a.sig").encode()
    assert engine.lib().ksp_sig_read(p, 21, None, None, 0, ctypes.byref(n), ctypes.byref(has)) == engine.KSP_E_OVERFLOW and (n.value, has.value) == (4, 1)
    room = np.full(4, 99, dtype=np.uint64)
    assert engine.lib().ksp_sig_read(p, 21, room.ctypes.data, None, 3, ctypes.byref(n), ctypes.byref(has)) == engine.KSP_E_ARG
    room32 = np.full(4, 99, dtype=np.uint32)
    assert engine.lib().ksp_sig_read(p, 21, room.ctypes.data, room32.ctypes.data, 3, ctypes.byref(n), ctypes.byref(has)) == engine.KSP_E_OVERFLOW
    assert n.value == 4 and (room == 99).all() and (room32 == 99).all()


def test_the_loader_of_a_directory_still_reads_signatures_with_abundances(samples, monkeypatch, tmp_path):
    """kspider_pack over counted signatures: the keys are the plain ones (abundances are not part of a pack)"""
    src, _ = samples
    _sketch_dir(monkeypatch, src, tmp_path / "counted", True)
    _sketch_dir(monkeypatch, src, tmp_path / "plain", False)
    engine.pack(str(tmp_path / "counted"), K, str(tmp_path / "c.pack"), 2)
    engine.pack(str(tmp_path / "plain"), K, str(tmp_path / "p.pack"), 2)
    assert open(tmp_path / "c.pack", "rb").read() == open(tmp_path / "p.pack", "rb").read()


# ---- the same code under the sanitizers, as a program of its own

def test_counted_driver_and_sig_reader_under_the_sanitizers(samples, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan-sketch"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=4096",
               UBSAN_OPTIONS="print_stacktrace=1", KSPIDER_SKETCH_BATCH_BYTES="1024")

    def run(*args):
        p = subprocess.run([EXE, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()

    src, seqs = samples
    lines = run("abund", src, str(K), str(SCALED), str(tmp_path / "sigs"))
    assert lines[-1].startswith("rc 0") and len(lines) == len(seqs) + 1
    for line, name in zip(lines, sorted(seqs)):
        (want,) = A.sketch(seqs[name], [0, len(seqs[name])], K, R.max_hash_of(SCALED))
        assert line.split() == ["sig", "0", str(len(want)), str(sum(n for _, n in want)), str(tmp_path / "sigs" / (name + ".sig"))]
    lines = run("abund", os.path.join(src, "repeat.fa"), "64", "1", str(tmp_path / "per"), "--per-record")
    assert lines[-1].startswith("rc 0") and [ln.split()[1] for ln in lines[:-1]] == ["0", "0"]
    # hostile signature files: a good one cut at every third byte, bytes flipped, lengths that disagree, deep nesting
    rng = random.Random(61)
    good = json.dumps([{"signatures": [{"ksize": K, "mins": [5, 3, 5, 2**64 - 1], "abundances": [1, 2**32 - 1, 7, 0]}]}]).encode()
    corpus = [good[:cut] for cut in range(0, len(good), 3)]
    for _ in range(40):
        b = bytearray(good)
        b[rng.randrange(len(b))] = rng.choice(b'[]{},:"0-9e\0\xff')
        corpus.append(bytes(b))
    corpus += [good.replace(b"[1, ", b"["), good.replace(b"[5, ", b"["), b"[" * 2000, b'[{"signatures":[{"ksize":21,"abundances":' + b"[" * 600, gzip.compress(good)[:20]]
    paths = []
    for i, blob in enumerate(corpus):
        p = tmp_path / f"h{i:03d}.sig"
        p.write_bytes(blob)
        paths.append(str(p))
    lines = run("sigs", str(K), *paths)
    assert len(lines) == len(paths)
    for path, line in zip(paths, lines):
        rc = int(line.split()[1])
        try:
            engine.sig_read(path, K)
            want = 0
        except engine.KspError as e:
            want = e.code
        assert rc == want and rc in (engine.KSP_OK, engine.KSP_E_IO), line
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "a.fa").write_text(">a\nACGTACGTACGT\n")
    (bad / "b.fq").write_text("@x\nACGT\n+\nII\n")
    assert run("abund", str(bad), "5", "1", str(tmp_path / "none"))[-1].startswith(f"rc {engine.KSP_E_IO}")
    assert not os.path.exists(tmp_path / "none")

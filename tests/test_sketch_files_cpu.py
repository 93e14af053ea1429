"""The file layer of the sketcher without a GPU: the FASTA / FASTQ reader (csrc/fastx_reader.cpp), the driver in host mode
(csrc/sketch_files.cpp with KSPIDER_SKETCH=host: .sig files, their md5sum, the batches), the way back through kspider_pack, and
the same code under AddressSanitizer + UBSan as a program of its own (`make -C kspider_amd/csrc asan-sketch`)."""
import gzip
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kspider_amd", "lib", "sketch_asan_check")
K, SCALED = 21, 4


def _fasta(records, width=60, eol="\n", final_newline=True):
    out = ""
    for name, seq in records:
        out += ">" + name + eol
        for i in range(0, len(seq), width):
            out += seq[i:i + width] + eol
    return out if final_newline else out[:-len(eol)]


def _fastq(records, eol="\n", final_newline=True, rng=None):
    rng = rng or random.Random(5)
    out = ""
    for i, (name, seq) in enumerate(records):
        qual = "".join(rng.choice("@>+IIFF#") for _ in seq)
        if seq:
            qual = "@>"[i % 2] + qual[1:]   # a quality line that looks like a header
        out += "@" + name + eol + seq + eol + "+" + eol + qual + eol
    return out if final_newline else out[:-len(eol)]


def _records(seed, n, lo=30, hi=400, lower=0.2):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = list(I.bases(rng, rng.randint(lo, hi), lower=lower))
        if len(s) > 50:
            s[rng.randrange(len(s))] = "N"
        out.append((f"r{seed}_{i} some description", "".join(s)))
    return out


def _seq_of(records):
    """What the reader hands on: every record's bases followed by one newline."""
    return "".join(seq + "\n" for _, seq in records).encode()


# ---- the reader

def _check_read(path, records, fastq):
    got = engine.fastx_read(str(path))
    assert got["seq"] == _seq_of(records)
    assert got["names"] == [name.split()[0] if name.split() else "" for name, _ in records]
    assert got["fastq"] == fastq
    off = [0]
    for _, s in records:
        off.append(off[-1] + len(s) + 1)
    assert got["rec_offsets"].tolist() == off


def test_reader_fasta_wrapped_crlf_empty_record_no_final_newline_lower_case(tmp_path):
    recs = _records(1, 5) + [("empty", "")] + _records(2, 2) + [("last", "acgtnACGT")]
    for i, (width, eol, final) in enumerate([(60, "\n", True), (7, "\r\n", True), (1000, "\n", False), (13, "\r\n", False)]):
        p = tmp_path / f"a{i}.fa"
        p.write_bytes(_fasta(recs, width, eol, final).encode())
        _check_read(p, recs, False)
    p = tmp_path / "ends_empty.fa"
    p.write_bytes(_fasta(recs[:2] + [("empty_at_end", "")], final_newline=False).encode())
    _check_read(p, recs[:2] + [("empty_at_end", "")], False)


def test_reader_fastq_with_header_like_quality_lines(tmp_path):
    recs = _records(3, 9) + [("none", "")]
    for i, (eol, final) in enumerate([("\n", True), ("\r\n", True), ("\n", False)]):
        p = tmp_path / f"q{i}.fq"
        p.write_bytes(_fastq(recs, eol, final).encode())
        _check_read(p, recs, True)


def test_reader_gzip_and_empty_file(tmp_path):
    recs = _records(4, 6)
    p = tmp_path / "a.fa.gz"
    p.write_bytes(gzip.compress(_fasta(recs).encode()))
    _check_read(p, recs, False)
    p = tmp_path / "q.fastq.gz"
    p.write_bytes(gzip.compress(_fastq(recs).encode()))
    _check_read(p, recs, True)
    p = tmp_path / "nothing.fa"
    p.write_bytes(b"\n\n")
    _check_read(p, [], False)


def test_reader_refuses_with_file_and_line(tmp_path):
    recs = _records(5, 4, lo=2000, hi=3000)
    whole = gzip.compress(_fasta(recs).encode())
    bad = {}
    (tmp_path / "cut.fa.gz").write_bytes(whole[:len(whole) // 2])
    bad["cut.fa.gz"] = "gzip"
    text = _fastq(recs)
    lines = text.split("\n")
    (tmp_path / "short.fq").write_text("\n".join(lines[:6]) + "\n")       # the second record has no '+' line
    bad["short.fq"] = "line 6"
    (tmp_path / "noqual.fq").write_text("\n".join(lines[:7]) + "\n")      # ... no quality line
    bad["noqual.fq"] = "line 7"
    (tmp_path / "qual.fq").write_text("\n".join(lines[:7] + [lines[7][:-1]]) + "\n")   # ... a quality line one byte short
    bad["qual.fq"] = "line 8"
    (tmp_path / "plus.fq").write_text("\n".join(lines[:2] + ["x"] + lines[3:]) + "\n")
    bad["plus.fq"] = "line 3"
    (tmp_path / "text.fa").write_text("hello\n>a\nACGT\n")
    bad["text.fa"] = "line 1"
    for name, what in bad.items():
        with pytest.raises(engine.KspError) as ei:
            engine.fastx_read(str(tmp_path / name))
        assert ei.value.code == engine.KSP_E_IO and name in str(ei.value) and what in str(ei.value), str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.fastx_read(str(tmp_path / "missing.fa"))
    assert ei.value.code == engine.KSP_E_IO


# ---- the driver in host mode

@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """A directory of FASTA / FASTQ / gz files, one of them with a record of 9 000 bases, and the records of every source."""
    d = tmp_path_factory.mktemp("genomes")
    rng = random.Random(9)
    g1, g2 = _records(11, 12), _records(12, 30, 40, 150)
    sources = {   # (g3 shares records with g1, g5 with g2: the pairwise table of the signatures has rows)
        "g1": (g1, "g1.fa", lambda r: _fasta(r).encode()),
        "g2": (g2, "g2.fastq", lambda r: _fastq(r).encode()),
        "g3": (_records(13, 8) + g1[:6], "g3.fna.gz", lambda r: gzip.compress(_fasta(r, 80, "\r\n").encode())),
        "g4": ([("long", I.bases(rng, 9000, lower=0.1))] + _records(14, 3), "g4.fasta", lambda r: _fasta(r, 70, "\n", False).encode()),
        "g5": (_records(15, 20, 40, 150) + g2[:10], "g5.fq.gz", lambda r: gzip.compress(_fastq(r).encode())),
        "g6": ([], "g6.fa", lambda r: b""),
    }
    (d / "notes.txt").write_text("not an input\n")
    for records, filename, make in sources.values():
        (d / filename).write_bytes(make(records))
    return str(d), {name: (records, filename) for name, (records, filename, _) in sources.items()}


@pytest.fixture(scope="module")
def restated(genomes):
    """name -> the restated sketch of every source of the directory."""
    mh = R.max_hash_of(SCALED)
    return {name: R.sketch(_seq_of(records), [0, len(_seq_of(records))], K, mh)[0] for name, (records, _) in genomes[1].items()}


def _sketch_dir(monkeypatch, genomes_dir, out, batch_bytes=None, threads=3):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    if batch_bytes:
        monkeypatch.setenv("KSPIDER_SKETCH_BATCH_BYTES", str(batch_bytes))
    engine.sketch_files(genomes_dir, K, SCALED, str(out), threads)
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


def test_host_mode_writes_signatures_that_json_reads(monkeypatch, genomes, restated, tmp_path):
    files = _sketch_dir(monkeypatch, genomes[0], tmp_path / "sigs")
    assert sorted(files) == sorted(name + ".sig" for name in genomes[1])
    for name, (records, filename) in genomes[1].items():
        doc = json.loads(files[name + ".sig"])
        assert isinstance(doc, list) and len(doc) == 1
        top = doc[0]
        assert top["class"] == "sourmash_signature" and top["hash_function"] == "0.murmur64" and top["filename"] == filename
        assert top["email"] == "" and top["license"] == "CC0" and top["version"] == 0.4
        (sig,) = top["signatures"]
        assert sig["num"] == 0 and sig["ksize"] == K and sig["seed"] == 42 and sig["max_hash"] == R.max_hash_of(SCALED) and sig["molecule"] == "DNA"
        assert sig["mins"] == restated[name]
        assert sig["md5sum"] == hashlib.md5((str(K) + "".join(str(m) for m in sig["mins"])).encode()).hexdigest()
    assert restated["g6"] == [] and len(restated["g4"]) > 1000


def test_small_batches_give_the_same_bytes(monkeypatch, genomes, tmp_path):
    """4 KiB batches: sources span batches, and the record of 9 000 bases is cut twice."""
    whole = _sketch_dir(monkeypatch, genomes[0], tmp_path / "whole")
    small = _sketch_dir(monkeypatch, genomes[0], tmp_path / "small", batch_bytes=4096)
    one_thread = _sketch_dir(monkeypatch, genomes[0], tmp_path / "one", batch_bytes=1024, threads=1)
    assert small == whole and one_thread == whole


def test_pack_reads_the_signatures_back(monkeypatch, genomes, restated, tmp_path):
    _sketch_dir(monkeypatch, genomes[0], tmp_path / "sigs")
    engine.pack(str(tmp_path / "sigs"), K, str(tmp_path / "db.pack"), 2)
    got = engine.pack_read(str(tmp_path / "db.pack"))
    assert got["ksize"] == K and got["names"] == sorted(genomes[1]) and got["present"].all()
    for g, name in enumerate(got["names"]):
        run = got["keys"][int(got["offsets"][g]):int(got["offsets"][g + 1])]
        assert run.tolist() == restated[name] and got["kmers"][g] == len(restated[name])


def test_per_record_mode_and_seed(monkeypatch, tmp_path):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    recs = [(f"read{i} x", s) for i, (_, s) in enumerate(_records(21, 15))]
    (tmp_path / "reads.fq").write_text(_fastq(recs))
    engine.sketch_files(str(tmp_path / "reads.fq"), 15, 2, str(tmp_path / "out"), 2, per_record=True, seed=7)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"read{i}.sig" for i in range(15))
    mh = R.max_hash_of(2)
    for i, (_, s) in enumerate(recs):
        sig = json.load(open(tmp_path / "out" / f"read{i}.sig"))[0]["signatures"][0]
        assert sig["seed"] == 7 and sig["mins"] == R.sketch((s + "\n").encode(), [0, len(s) + 1], 15, mh, seed=7)[0]
    # the same file as one source: the union
    engine.sketch_files(str(tmp_path / "reads.fq"), 15, 2, str(tmp_path / "one"), 2, seed=7)
    sig = json.load(open(tmp_path / "one" / "reads.sig"))[0]["signatures"][0]
    assert sig["mins"] == R.sketch(_seq_of(recs), [0, len(_seq_of(recs))], 15, mh, seed=7)[0]


def test_driver_refusals(monkeypatch, genomes, tmp_path):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    out = str(tmp_path / "o")
    for args in [(genomes[0], 0, 4, out), (genomes[0], 65, 4, out), (genomes[0], 21, 0, out), ("", 21, 4, out), (genomes[0], 21, 4, "")]:
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_files(*args)
        assert ei.value.code == engine.KSP_E_ARG
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_files(str(empty), 21, 4, out)
    assert ei.value.code == engine.KSP_E_IO
    twins = tmp_path / "twins"
    twins.mkdir()
    (twins / "a.fa").write_text(">x\nACGT\n")
    (twins / "a.fq").write_text("@x\nACGT\n+\nIIII\n")
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_files(str(twins), 3, 1, out)
    assert ei.value.code == engine.KSP_E_ARG and "named a" in str(ei.value)
    monkeypatch.setenv("KSPIDER_SKETCH", "elsewhere")
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_files(genomes[0], 21, 4, out)
    assert ei.value.code == engine.KSP_E_ARG
    assert not os.path.exists(out)


# ---- the same code under the sanitizers, as a program of its own

def test_reader_and_driver_under_the_sanitizers(genomes, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan-sketch"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=4096",
               UBSAN_OPTIONS="print_stacktrace=1", KSPIDER_SKETCH_BATCH_BYTES="2048")

    def run(*args):
        p = subprocess.run([EXE, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()

    # hostile inputs: a good FASTQ cut at every byte of its first records, bytes flipped, a cut gzip, binary noise
    rng = random.Random(31)
    good = _fastq(_records(32, 3, 20, 60)).encode()
    corpus = []
    for cut in range(0, min(len(good), 260), 3):
        corpus.append(good[:cut])
    for _ in range(40):
        b = bytearray(good)
        b[rng.randrange(len(b))] = rng.choice(b"@>+\n\r\0\xff")
        corpus.append(bytes(b))
    gz = gzip.compress(_fasta(_records(33, 4)).encode())
    corpus += [gz[:cut] for cut in (0, 5, 10, 18, len(gz) // 2, len(gz) - 1)]
    corpus += [bytes(rng.randrange(256) for _ in range(300)), b">", b"@", b">\n", b"@\n\n+\n", b"\r\n\r\n>a\r\nAC\r\n\r\nGT", b">a\n" + b"A" * 100000]
    paths = []
    for i, blob in enumerate(corpus):
        p = tmp_path / f"c{i:03d}.fq"
        p.write_bytes(blob)
        paths.append(str(p))
    lines = run("read", *paths)
    assert len(lines) == len(paths)
    for path, line in zip(paths, lines):
        rc = int(line.split()[0])
        try:
            engine.fastx_read(path)
            want = 0
        except engine.KspError as e:
            want = e.code
        assert rc == want and rc in (engine.KSP_OK, engine.KSP_E_IO), line
    # the driver: small batches, per file and per record, and a directory with a bad file in it
    assert run("sketch", genomes[0], str(K), str(SCALED), str(tmp_path / "sigs"))[-1].startswith("rc 0")
    whole = {f: open(tmp_path / "sigs" / f, "rb").read() for f in os.listdir(tmp_path / "sigs")}
    assert len(whole) == len(genomes[1])
    for name, (records, _) in genomes[1].items():
        mins = json.loads(whole[name + ".sig"])[0]["signatures"][0]["mins"]
        assert mins == R.sketch(_seq_of(records), [0, len(_seq_of(records))], K, R.max_hash_of(SCALED))[0]
    assert run("sketch", os.path.join(genomes[0], "g2.fastq"), "64", "1", str(tmp_path / "per"), "--per-record")[-1].startswith("rc 0")
    assert len(os.listdir(tmp_path / "per")) == 30
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "a.fa").write_text(">a\nACGTACGTACGT\n")
    (bad / "b.fq").write_bytes(good[:len(good) - 30])
    assert run("sketch", str(bad), "5", "1", str(tmp_path / "none"))[-1].startswith(f"rc {engine.KSP_E_IO}")
    assert not os.path.exists(tmp_path / "none")

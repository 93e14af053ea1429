"""Protein, dayhoff and hp sketches without a GPU: ksp_sketch_cpu_mol and ksp_sketch_text_hash against the
restatement (tests/sketch_protein_restate.py), the refusals, the file driver in host mode (batches, cuts in every codon phase,
the .sig fields, the way back through ksp_sig_read, DNA output unchanged), and the sanitizer program's new mode."""
import ctypes
import functools
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import sketch_inputs as DI
import sketch_protein_inputs as I
import sketch_protein_restate as P
import sketch_restate as R
from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kspider_amd", "lib", "sketch_asan_check")
FULL = 2**64 - 1
FEW = P.max_hash_of(25)   # keeps four percent
MOLS = [P.PROTEIN, P.DAYHOFF, P.HP]


def _same(case, k, mol, translated, max_hash=FULL):
    want = P.flat(P.counted_sketch(case.seq, case.offsets, k, mol, translated, max_hash))
    keys, abund, off = engine.sketch_cpu_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash, abund=True)
    assert (off == want[2]).all() and (keys == want[0]).all() and (abund == want[1]).all(), (case.name, k, mol, translated)
    plain_keys, plain_off = engine.sketch_cpu_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash)
    assert (plain_keys == keys).all() and (plain_off == off).all()
    return keys, abund, off


@functools.lru_cache(maxsize=None)
def _protein_mixed():
    return I.protein_mixed()


@functools.lru_cache(maxsize=None)
def _dna_mixed():
    return I.dna_mixed()


@pytest.mark.parametrize("mol", MOLS)
@pytest.mark.parametrize("k", I.RESIDUE_K)
def test_protein_input(k, mol):
    for max_hash in (FULL, FEW):
        _same(_protein_mixed(), k, mol, False, max_hash)


@pytest.mark.parametrize("mol", MOLS)
@pytest.mark.parametrize("k", I.TRANSLATED_K)
def test_translated_input(k, mol):
    for max_hash in (FULL, FEW):
        _same(_dna_mixed(), k, mol, True, max_hash)


@pytest.mark.parametrize("k", [1, 9, 33, 64])
def test_all_256_byte_values_as_protein_input(k):
    c = I.all_byte_values()
    for mol in MOLS:
        keys, _, _ = _same(c, k, mol, False)
        assert keys.size > 0
    # a lower-case stream and its upper-case twin: the same sketch
    lower = DI.Case("lower", c.seq.lower(), c.offsets)
    upper = DI.Case("upper", c.seq.upper(), c.offsets)
    a, b = _same(lower, k, P.PROTEIN, False), _same(upper, k, P.PROTEIN, False)
    assert all((x == y).all() for x, y in zip(a, b))


def test_text_hash_and_the_star():
    for mol in MOLS:
        for text in ("M", "MKV*LLA", "mkv*lla", "ACDEFGHIKLMNPQRSTVWYBJOUXZ*", "W" * 64):
            h, valid = engine.sketch_text_hash(text, mol)
            assert valid and h == P.text_hashes([P.encode(text, mol)])[0], (mol, text)
        for text in ("MK-V", "MKV\n", "M1", "\0"):
            assert engine.sketch_text_hash(text, mol) == (0, False)
    keys, abund, _ = engine.sketch_cpu_mol(b"MK*VMK*V", [0, 8], 3, "protein", max_hash=FULL, abund=True)
    want = P.counted_sketch(b"MK*VMK*V", [0, 8], 3, P.PROTEIN, False, FULL)[0]
    assert dict(zip(keys.tolist(), abund.tolist())) == want and engine.sketch_text_hash("K*V", 1)[0] in want
    for bad in [("MKV", 0), ("MKV", 4), ("", 1), ("M" * 65, 1)]:
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_text_hash(*bad)
        assert ei.value.code == engine.KSP_E_ARG


@pytest.mark.parametrize("k", I.TRANSLATED_K)
def test_a_break_byte_at_every_offset_of_a_window(k):
    _same(I.break_at_every_offset(k), k, P.PROTEIN, True)


@pytest.mark.parametrize("k,translated", [(1, True), (10, True), (21, True), (1, False), (33, False), (64, False)])
def test_abutting_sources_and_a_source_shorter_than_the_window(k, translated):
    window = 3 * k if translated else k
    for c in I.abutting(window, dna=translated):
        keys, abund, off = _same(c, k, P.DAYHOFF, translated)
        assert off[3] == off[2] and off[1] == 0      # the short source and the empty ones have no k-mer
        one = P.counted_sketch(c.seq, [0, len(c.seq)], k, P.DAYHOFF, translated, FULL)[0]
        assert sum(one.values()) > int(abund.sum()) or window == 1   # as one source the seams' windows are there


@pytest.mark.parametrize("k", [2, 10])
def test_a_window_whose_strands_translate_alike_counts_twice(k):
    keys, abund, _ = _same(I.alike_on_both_strands(k), k, P.PROTEIN, True)
    assert keys.size == 1 and abund.tolist() == [2]


def test_refusals():
    c = _dna_mixed()
    cases = [(22, P.PROTEIN, True, "21"), (0, P.PROTEIN, True, "21"), (65, P.PROTEIN, False, "64"), (0, P.HP, False, "64"), (10, 0, True, "TRANSLATE"), (10, 4, False, "moltype"),
             (10, -1, False, "moltype")]
    for k, mol, translated, what in cases:
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_cpu_mol(c.seq, c.offsets, k, mol, translated, max_hash=FULL)
        assert ei.value.code == engine.KSP_E_ARG and what in str(ei.value), str(ei.value)
    L = engine.lib()
    off = np.array([0, 10], dtype=np.uint64)
    needed = ctypes.c_uint64(0)
    assert L.ksp_sketch_cpu_mol(b"ACGTACGTAC", 10, off.ctypes.data, 1, 2, 1, 128, FULL, 42, None, None, 0, off.ctypes.data, ctypes.byref(needed)) == engine.KSP_E_ARG


def test_moltype_0_is_the_dna_call():
    c = DI.mixed()
    for k in (1, 21, 33, 64):
        keys, abund, off = engine.sketch_cpu_mol(c.seq, c.offsets, k, 0, max_hash=FEW, abund=True)
        want = engine.sketch_cpu_abund(c.seq, c.offsets, k, max_hash=FEW)
        assert (keys == want[0]).all() and (abund == want[1]).all() and (off == want[2]).all()


@pytest.mark.parametrize("k", [1, 7, 11, 21])
def test_translated_equals_protein_input_of_the_six_frames(k):
    """Windows free of breaks: one record of bases.  The six frame translations as six sources' worth of protein input, separated
    by breaks, sketched as one source at scaled 1: the same set of hashes."""
    dna = DI.bases(random.Random(60 + k), 400, lower=0.2)
    keys, _ = engine.sketch_cpu_mol(dna.encode(), [0, len(dna)], k, P.PROTEIN, True, max_hash=FULL)
    frames = [P.translate(s[f:]) for s in (dna, P.revcomp(dna)) for f in range(3)]
    protein = "\n".join(frames).encode()
    want, _ = engine.sketch_cpu_mol(protein, [0, len(protein)], k, P.PROTEIN, False, max_hash=FULL)
    assert keys.size > 0 and (keys == want).all()


# ---- the file driver in host mode

def _fasta(records, width=60):
    return "".join(">" + name + "\n" + "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width)) for name, seq in records)


def _seq_of(records):
    return "".join(seq + "\n" for _, seq in records).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """A directory of genomes (one record of 9 000 bases: with 1 KiB batches it is cut in every codon phase) and one of proteomes
    (a record of 5 000 residues; a .faa, a .fa and a .fasta file, and a .fna file that protein mode must not pick up)."""
    rng = random.Random(70)
    g = tmp_path_factory.mktemp("genomes")
    genomes = {"g1": [("long", DI.bases(rng, 9000, lower=0.1)), ("b", DI.bases(rng, 300) + "N" + DI.bases(rng, 200))],
               "g2": [(f"r{i}", DI.bases(rng, rng.randint(20, 300))) for i in range(12)]}
    genomes["g3"] = genomes["g2"][:6] + [("own", DI.bases(rng, 700))]
    for name, ending in (("g1", ".fa"), ("g2", ".fna"), ("g3", ".fasta")):
        (g / (name + ending)).write_text(_fasta(genomes[name]))
    p = tmp_path_factory.mktemp("proteomes")
    proteomes = {"p1": [("long", I.residues(rng, 5000, lower=0.1)), ("s", "MKV*LLX" + I.residues(rng, 100))],
                 "p2": [(f"q{i}", I.residues(rng, rng.randint(5, 200))) for i in range(15)]}
    proteomes["p3"] = proteomes["p2"][:8] + [("own", I.residues(rng, 300))]
    for name, ending in (("p1", ".faa"), ("p2", ".fa"), ("p3", ".fasta")):
        (p / (name + ending)).write_text(_fasta(proteomes[name]))
    (p / "dna.fna").write_text(">x\nACGT\n")
    return str(g), genomes, str(p), proteomes


def _sketch_dir(monkeypatch, src, k, scaled, out, batch_bytes=None, threads=2, **kw):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    if batch_bytes:
        monkeypatch.setenv("KSPIDER_SKETCH_BATCH_BYTES", str(batch_bytes))
    else:
        monkeypatch.delenv("KSPIDER_SKETCH_BATCH_BYTES", raising=False)
    engine.sketch_files(src, k, scaled, str(out), threads, **kw)
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


def _check_sigs(files, records_of, k, scaled, mol, translated):
    assert sorted(files) == sorted(n + ".sig" for n in records_of)
    for name, records in records_of.items():
        (sig,) = json.loads(files[name + ".sig"])[0]["signatures"]
        seq = _seq_of(records)
        want = P.counted_sketch(seq, [0, len(seq)], k, mol, translated, P.max_hash_of(scaled))[0]
        assert sig["molecule"] == P.NAMES[mol] and sig["ksize"] == 3 * k and sig["num"] == 0 and sig["seed"] == 42 and sig["max_hash"] == P.max_hash_of(scaled)
        assert sig["mins"] == sorted(want) and len(want) > 0
        assert sig["abundances"] == [want[h] for h in sorted(want)]
        assert sig["md5sum"] == hashlib.md5((str(3 * k) + "".join(str(m) for m in sig["mins"])).encode()).hexdigest()


@pytest.mark.parametrize("mol", MOLS)
def test_translated_files_do_not_depend_on_the_batch_size(monkeypatch, inputs, tmp_path, mol):
    """1 024-byte batches cut the 9 000-base record eight times, with 3k - 1 = 29 bytes of overlap; the cuts fall at 995 n + const,
    and 995 = 3 * 331 + 2, so they fall in every codon phase.  Counts across the cuts stay exact."""
    g, genomes = inputs[0], inputs[1]
    whole = _sketch_dir(monkeypatch, g, 10, 2, tmp_path / "whole", moltype=mol, translate=True, abund=True)
    _check_sigs(whole, genomes, 10, 2, mol, True)
    for batch in (1024, 1500, 4096):
        assert _sketch_dir(monkeypatch, g, 10, 2, tmp_path / f"b{batch}", batch_bytes=batch, threads=1, moltype=mol, translate=True, abund=True) == whole
    plain = _sketch_dir(monkeypatch, g, 10, 2, tmp_path / "plain", batch_bytes=1024, moltype=mol, translate=True)
    for name in genomes:
        a, b = json.loads(plain[name + ".sig"])[0]["signatures"][0], json.loads(whole[name + ".sig"])[0]["signatures"][0]
        assert "abundances" not in a and a["mins"] == b["mins"] and a["md5sum"] == b["md5sum"]


@pytest.mark.parametrize("mol", MOLS)
def test_protein_files(monkeypatch, inputs, tmp_path, mol):
    p, proteomes = inputs[2], inputs[3]
    whole = _sketch_dir(monkeypatch, p, 7, 3, tmp_path / "whole", moltype=P.NAMES[mol], abund=True)
    _check_sigs(whole, proteomes, 7, 3, mol, False)      # (and dna.fna was not picked up)
    assert _sketch_dir(monkeypatch, p, 7, 3, tmp_path / "small", batch_bytes=1024, threads=1, moltype=mol, abund=True) == whole
    for name, records in proteomes.items():
        mins, abunds = engine.sig_read(str(tmp_path / "whole" / (name + ".sig")), 21)
        sig = json.loads(whole[name + ".sig"])[0]["signatures"][0]
        assert mins.tolist() == sig["mins"] and abunds.tolist() == sig["abundances"]
        with pytest.raises(engine.KspError):
            engine.sig_read(str(tmp_path / "whole" / (name + ".sig")), 7)


def test_dna_output_is_what_it_was(monkeypatch, inputs, tmp_path):
    """Without the new flags: the bytes the DNA definition gives, "molecule":"DNA" and "ksize": K, at two batch sizes."""
    g, genomes = inputs[0], inputs[1]
    whole = _sketch_dir(monkeypatch, g, 21, 4, tmp_path / "whole")
    assert _sketch_dir(monkeypatch, g, 21, 4, tmp_path / "small", batch_bytes=1024) == whole
    for name, records in genomes.items():
        seq = _seq_of(records)
        mins = R.sketch(seq, [0, len(seq)], 21, R.max_hash_of(4))[0]
        md5 = hashlib.md5(("21" + "".join(str(m) for m in mins)).encode()).hexdigest()
        filename = {"g1": "g1.fa", "g2": "g2.fna", "g3": "g3.fasta"}[name]
        want = ('[{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":"' + filename + '","license":"CC0","version":0.4,"signatures":[{"num":0,'
                '"ksize":21,"seed":42,"max_hash":' + str(R.max_hash_of(4)) + ',"molecule":"DNA","md5sum":"' + md5 + '","mins":[' + ",".join(str(m) for m in mins) + "]}]}]\n")
        assert whole[name + ".sig"].decode() == want


def test_driver_refusals(monkeypatch, inputs, tmp_path):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    g, out = inputs[0], str(tmp_path / "o")
    L = engine.lib()
    for k, flags, what in [(10, engine.SKETCH_PROTEIN | engine.SKETCH_HP, "exclude"), (10, engine.SKETCH_DAYHOFF | engine.SKETCH_HP | engine.SKETCH_TRANSLATE, "exclude"),
                           (10, engine.SKETCH_TRANSLATE, "needs"), (22, engine.SKETCH_PROTEIN | engine.SKETCH_TRANSLATE, "21"), (65, engine.SKETCH_PROTEIN, "64"),
                           (0, engine.SKETCH_HP, "64")]:
        assert L.kspider_sketch(g.encode(), k, 2, out.encode(), 1, flags) == engine.KSP_E_ARG
        assert what in L.ksp_last_error().decode()
    with pytest.raises(ValueError):
        engine.sketch_files(g, 10, 2, out, moltype="rna")
    with pytest.raises(engine.KspError) as ei:   # protein mode finds no .faa / .fa / .fasta file in a directory of .fna files
        only_fna = tmp_path / "fna"
        only_fna.mkdir()
        (only_fna / "a.fna").write_text(">x\nACGT\n")
        engine.sketch_files(str(only_fna), 3, 1, out, moltype="protein")
    assert ei.value.code == engine.KSP_E_IO and ".faa" in str(ei.value)
    assert not os.path.exists(out)


# ---- the same code under the sanitizers, as a program of its own

def test_the_driver_with_the_new_flags_under_the_sanitizers(inputs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kspider_amd", "csrc"), "asan-sketch"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=4096",
               UBSAN_OPTIONS="print_stacktrace=1", KSPIDER_SKETCH_BATCH_BYTES="1024")

    def run(*args):
        p = subprocess.run([EXE, *args], capture_output=True, text=True, env=env, timeout=120)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()

    # hostile protein files: every byte value, lines of stars and breaks only, a record of one residue, an empty record, a long
    # record without a newline at its end, binary noise behind a header
    rng = random.Random(71)
    hostile = tmp_path / "hostile"
    hostile.mkdir()
    (hostile / "bytes.faa").write_bytes(b">all\n" + bytes(b for b in range(256) if b not in (10, 13, 62)) * 9 + b"\n")
    (hostile / "stars.faa").write_bytes(b">s\n*******\n-------\n*\n>one\nM\n>none\n>last\n" + I.residues(rng, 3000).encode())
    (hostile / "noise.fa").write_bytes(b">n\n" + bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWY*\0\xff\t ") for _ in range(5000)) + b"\n")
    flags = engine.SKETCH_ABUND
    for moltype, k in ((engine.SKETCH_PROTEIN, 64), (engine.SKETCH_DAYHOFF, 17), (engine.SKETCH_HP, 1)):
        out = tmp_path / f"h{moltype}"
        lines = run("mol", str(flags | moltype), str(hostile), str(k), "1", str(out))
        assert lines[-1].startswith("rc 0") and len(lines) == 4 and all(l.startswith("sig 0 ") for l in lines[:3]), lines
        for name in ("bytes", "stars", "noise"):
            seq = engine.fastx_read(str(hostile / (name + (".fa" if name == "noise" else ".faa"))))["seq"]
            want = P.counted_sketch(seq, [0, len(seq)], k, {8: 1, 16: 2, 32: 3}[moltype], False, FULL)[0]
            (sig,) = json.loads(open(out / (name + ".sig")).read())[0]["signatures"]
            assert sig["mins"] == sorted(want) and sig["abundances"] == [want[h] for h in sorted(want)]
    # translated, per record, over the genomes; and a refusal that writes nothing
    g, genomes = inputs[0], inputs[1]
    lines = run("mol", str(flags | engine.SKETCH_PROTEIN | engine.SKETCH_TRANSLATE), g, "21", "1", str(tmp_path / "t"))
    assert lines[-1].startswith("rc 0") and len(lines) == 4
    (sig,) = json.loads(open(tmp_path / "t" / "g1.sig").read())[0]["signatures"]
    seq = _seq_of(genomes["g1"])
    want = P.counted_sketch(seq, [0, len(seq)], 21, P.PROTEIN, True, FULL)[0]
    assert sig["ksize"] == 63 and sig["mins"] == sorted(want) and sig["abundances"] == [want[h] for h in sorted(want)]
    lines = run("mol", str(engine.SKETCH_HP | engine.SKETCH_TRANSLATE | engine.SKETCH_PER_RECORD), os.path.join(g, "g2.fna"), "2", "1", str(tmp_path / "per"))
    assert lines[-1].startswith("rc 0") and len(os.listdir(tmp_path / "per")) == 12
    lines = run("mol", str(engine.SKETCH_TRANSLATE), g, "10", "1", str(tmp_path / "none"))
    assert lines[-1].startswith(f"rc {engine.KSP_E_ARG}") and not os.path.exists(tmp_path / "none")

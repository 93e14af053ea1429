"""The weighted file path on the GPU, end to end: `sketch --abund` over a few small synthetic genomes and a sample of reads with
planted depths, then `gather --abund` on those signatures (kspider_gather_abund, kspider_amd/csrc/sketch_pack.cpp).  The TSV is
compared byte for byte with one written here from the restatements (tests/sketch_abund_restate.py, tests/gather_abund_restate.py)
and engine.format_float; its first nine columns are kspider_gather's file; a refused call leaves no file."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import gather_abund_restate as WR
import sketch_abund_restate as A
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu
K, SCALED, MIN_HASHES = 21, 2, 3
DEPTHS = {"g0": 30, "g2": 3, "g3": 9}       # genome -> the depth at which the sample holds it (g1 and g4 are not in it)
LIB = os.path.dirname(engine.LIB_PATH)
HEADER = ("query\trank\tmatch\toverlap\tunique\tf_orig_query\tf_unique_to_query\tf_match\tremaining\tf_unique_weighted\taverage_abund\tmedian_abund\tstd_abund\t"
          "n_unique_weighted_found\tsum_weighted_found\ttotal_weighted_hashes\n")


def _fasta(records):
    return "".join(">" + name + "\n" + seq + "\n" for name, seq in records)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """(root, the genomes' texts, the samples' texts): five genomes of 1 500 bases — g1 shares its first 500 with g0 —, sample s0 =
    reads of 100 bases from g0, g2 and g3 at the depths of DEPTHS, sample s1 = g4 once, whole"""
    root = tmp_path_factory.mktemp("planted")
    rng = random.Random(71)
    genomes = {f"g{i}": I.bases(rng, 1500) for i in range(5)}
    genomes["g1"] = genomes["g0"][:500] + genomes["g1"][500:]
    reads = []
    for g, depth in DEPTHS.items():
        for _ in range(depth * 1500 // 100):
            at = rng.randrange(1400)
            r = genomes[g][at:at + 100]
            reads.append(R.revcomp(r) if rng.random() < 0.5 else r)
    rng.shuffle(reads)
    samples = {"s0": [(f"r{i}", r) for i, r in enumerate(reads)], "s1": [("whole", genomes["g4"])]}
    (root / "genomes").mkdir()
    (root / "samples").mkdir()
    for name, text in genomes.items():
        (root / "genomes" / (name + ".fa")).write_text(_fasta([(name, text)]))
    for name, recs in samples.items():
        (root / "samples" / (name + ".fa")).write_text(_fasta(recs))
    return root, {n: (t + "\n").encode() for n, t in genomes.items()}, {n: "".join(s + "\n" for _, s in recs).encode() for n, recs in samples.items()}


def _expected(genomes, samples):
    mh = R.max_hash_of(SCALED)
    db_names, q_names = sorted(genomes), sorted(samples)
    db = [[h for h, _ in A.sketch(genomes[n], [0, len(genomes[n])], K, mh)[0]] for n in db_names]
    q_runs = [A.sketch(samples[n], [0, len(samples[n])], K, mh)[0] for n in q_names]
    q, a = [[h for h, _ in run] for run in q_runs], [[c for _, c in run] for run in q_runs]
    text, rows = _tsv(db, q, a, db_names, q_names)
    return text, rows, db_names


def _tsv(db, q, a, db_names, q_names, min_hashes=MIN_HASHES):
    """(the file of the weighted gather over the runs db, the runs q and their abundances a; the restatement's rows)"""
    text, rows = HEADER, WR.gather(db, q, a, min_hashes, 0)
    for row in rows:
        query, rank, source, overlap, unique, remaining, w_unique, w_found = row[:8]
        W = sum(a[query])
        floats = [np.float32(overlap) / np.float32(len(q[query])), np.float32(unique) / np.float32(len(q[query])), np.float32(overlap) / np.float32(len(db[source]))]
        weighted = [np.float32(v) for v in WR.columns(row, W)]
        text += "\t".join([q_names[query], str(rank), db_names[source], str(overlap), str(unique)] + [engine.format_float(float(v)) for v in floats] + [str(remaining)]
                          + [engine.format_float(float(v)) for v in weighted] + [str(w_unique), str(w_found), str(W)]) + "\n"
    return text.encode(), rows


def test_sketch_abund_then_gather_abund(planted):
    root, genomes, samples = planted
    engine.sketch_files(str(root / "genomes"), K, SCALED, str(root / "db_sigs"), 2)                         # the database: plain signatures
    done = subprocess.run([os.path.join(LIB, "sketch"), str(root / "samples"), str(K), str(SCALED), str(root / "q_sigs"), "2", "--abund"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    for name, seq in samples.items():                                                                        # counted on the device
        (want,) = A.sketch(seq, [0, len(seq)], K, R.max_hash_of(SCALED))
        sig = json.load(open(root / "q_sigs" / (name + ".sig")))[0]["signatures"][0]
        assert sig["mins"] == [h for h, _ in want] and sig["abundances"] == [c for _, c in want]
    want, rows, db_names = _expected(genomes, samples)
    by_match = {db_names[r[2]]: r for r in rows if r[0] == 0}
    assert set(by_match) >= set(DEPTHS) and [db_names[r[2]] for r in rows if r[0] == 1] == ["g4"]
    assert by_match["g0"][9] > by_match["g3"][9] > by_match["g2"][9]                                        # the planted depths show in the medians
    out = str(root / "OUT")
    engine.gather_abund(str(root / "db_sigs"), str(root / "q_sigs"), K, out, 2, min_hashes=MIN_HASHES)
    got = open(out + "_kSpider_gather.tsv", "rb").read()
    assert got == want
    engine.gather(str(root / "db_sigs"), str(root / "q_sigs"), K, out + "_plain", 2, min_hashes=MIN_HASHES)
    plain = open(out + "_plain_kSpider_gather.tsv", "rb").read()
    assert [ln.split(b"\t")[:9] for ln in got.splitlines()] == [ln.split(b"\t") for ln in plain.splitlines()]
    # the executable, and abundances in the database (ignored)
    engine.sketch_files(str(root / "genomes"), K, SCALED, str(root / "db_counted"), 2, abund=True)
    done = subprocess.run([os.path.join(LIB, "gather"), str(root / "db_counted"), str(root / "q_sigs"), str(K), out + "_tool", "2", str(MIN_HASHES), "--abund"],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert open(out + "_tool_kSpider_gather.tsv", "rb").read() == want
    assert not [f for f in os.listdir(root) if f.endswith(".partial")]


def test_device_batches_and_host_mode_write_the_same_bytes(planted, monkeypatch):
    """2 KiB batches on the device — the sample's reads span dozens of them, so the counts of a hash come from many segments and
    are added — and KSPIDER_SKETCH=host: byte for byte the files of one batch on the device"""
    root, _, samples = planted

    def files(out, **env):
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        engine.sketch_files(str(root / "samples"), K, SCALED, str(root / out), 2, abund=True)
        for name in env:
            monkeypatch.delenv(name)
        return {f: open(root / out / f, "rb").read() for f in sorted(os.listdir(root / out))}
    whole = files("whole")
    assert sorted(whole) == [n + ".sig" for n in sorted(samples)]
    assert files("small", KSPIDER_SKETCH_BATCH_BYTES="2048") == whole
    assert files("host", KSPIDER_SKETCH="host") == whole
    assert max(json.loads(whole["s0.sig"])[0]["signatures"][0]["abundances"]) > 20


def test_refusals_leave_no_file(planted):
    root, genomes, samples = planted
    for d in ("db_sigs", "q_sigs"):
        if not (root / d).exists():
            engine.sketch_files(str(root / ("genomes" if d == "db_sigs" else "samples")), K, SCALED, str(root / d), 2, abund=d == "q_sigs")
    engine.pack(str(root / "q_sigs"), K, str(root / "q.kspack"), 2)
    out = str(root / "NO")
    for queries, what in ((str(root / "q.kspack"), "q.kspack"), (str(root / "db_sigs"), "g0")):      # a pack file; signatures without abundances
        with pytest.raises(engine.KspError) as ei:
            engine.gather_abund(str(root / "db_sigs"), queries, K, out, 2, min_hashes=MIN_HASHES)
        assert ei.value.code == engine.KSP_E_ARG and what in str(ei.value) and "kspider_gather_abund" in str(ei.value), str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.gather_abund(str(root / "db_sigs"), str(root / "q_sigs"), K, out, 2, min_hashes=0)
    assert ei.value.code == engine.KSP_E_ARG
    assert not os.path.exists(out + "_kSpider_gather.tsv") and not os.path.exists(out + "_kSpider_gather.tsv.partial")

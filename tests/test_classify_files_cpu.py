"""The file driver of classify without a GPU (csrc/classify_files.cpp with KSPIDER_CLASSIFY=host): FASTA and FASTQ, gzip, a
directory and a single file, repeated names, a database directory and its pack; both TSV files byte for byte against text made
from the restatement (tests/classify_restate.py); the batch sizes; and the cross-check that defines the feature — per-record
ksp_sketch_cpu plus a set intersection gives the same hits."""
import os
import subprocess

import pytest

import classify_inputs as CI
import classify_restate as CR
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SCALED, MH = CI.FILES_K, CI.FILES_SCALED, CI.FILES_MH
REF_IDS, REF_NAMES, CUT = CI.REF_IDS, CI.FILE_REF_NAMES, CI.CUT


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return CI.files_world(tmp_path_factory.mktemp("classify_files"))


def _want(world, min_hits=1, records=None):
    lo, hi = records or (0, len(world["names"]))
    res = CR.from_kept(world["kept"][lo:hi], world["refs"], min_hits)
    return CR.summary_tsv(world["names"][lo:hi], world["lengths"][lo:hi], res, REF_NAMES), CR.hits_tsv(world["names"][lo:hi], res, REF_NAMES, REF_IDS)


def _run(world, monkeypatch, out, input_path=None, db=None, min_hits=1, batch=None, threads=2):
    monkeypatch.setenv("KSPIDER_CLASSIFY", "host")
    monkeypatch.delenv("KSPIDER_CLASSIFY_BATCH_BYTES", raising=False)
    if batch:
        monkeypatch.setenv("KSPIDER_CLASSIFY_BATCH_BYTES", str(batch))
    prefix = str(world["dir"] / out)
    engine.classify_files(str(input_path or world["reads"]), K, SCALED, str(db or world["db"]), prefix, threads, min_hits)
    return open(prefix + "_kSpider_classify.tsv").read(), open(prefix + "_kSpider_classify_hits.tsv").read()


def test_directory_of_fasta_and_gzipped_fastq_against_a_sig_directory(world, monkeypatch):
    summary, hits = _run(world, monkeypatch, "dir")
    want_summary, want_hits = _want(world)
    assert summary == want_summary and hits == want_hits
    assert len(hits.splitlines()) > 10 and "\t-\t0\t0\n" in summary and "contig/1\t" in summary   # a name keeps its '/'
    assert not [f for f in os.listdir(world["dir"]) if f.endswith(".partial")]


def test_batch_sizes_give_identical_files(world, monkeypatch):
    want = _want(world)
    assert _run(world, monkeypatch, "b1024", batch=1024) == want
    assert _run(world, monkeypatch, "bcut", batch=CUT) == want     # the cut lies inside the second copy of the repeated k-mer
    assert _run(world, monkeypatch, "bdefault") == want
    assert _run(world, monkeypatch, "b1025_one_thread", batch=1025, threads=1) == want
    # the repeated k-mer counts once: the long record's kept windows exceed its distinct hashes by the repeat (when it is kept)
    windows = world["kept"][0]
    x_hash = R.source_hashes(world["seq"][700:700 + K], K)[0]
    assert len(windows) - len(set(windows)) == (1 if x_hash <= MH else 0)


def test_single_file_pack_and_min_hits(world, monkeypatch):
    n = world["n_first"]
    assert _run(world, monkeypatch, "one", input_path=world["reads"] / "a.fa") == _want(world, records=(0, n))
    pack = str(world["dir"] / "db.pack")
    engine.pack(str(world["db"]), K, pack, 2)
    assert _run(world, monkeypatch, "pack", db=pack) == _want(world)
    rows = CR.from_kept(world["kept"], world["refs"])["rows"]
    m = CI.middle_hits(rows)
    for min_hits in (m - 1, m, m + 1):
        assert _run(world, monkeypatch, f"m{min_hits}", min_hits=min_hits, batch=2048) == _want(world, min_hits)


def test_hits_equal_per_record_sketches_intersected(world, monkeypatch):
    _, hits = _run(world, monkeypatch, "cross")
    keys, off = engine.sketch_cpu(world["seq"], world["off"], K, scaled=SCALED)
    want = []
    for r in range(len(world["names"])):
        mine = set(keys[int(off[r]):int(off[r + 1])].tolist())
        for q, ref in enumerate(world["refs"]):
            shared = len(mine & set(ref))
            if shared:
                want.append(f"{r + 1}\t{world['names'][r]}\t{REF_IDS[q]}\t{REF_NAMES[q]}\t{shared}\n")
    assert hits == "record_id\tname\tref_id\tref_name\thits\n" + "".join(want)


def test_the_exe_in_host_mode(world, monkeypatch):
    exe = os.path.join(ROOT, "kspider_amd", "lib", "classify")
    prefix = str(world["dir"] / "exe")
    env = dict(os.environ, KSPIDER_CLASSIFY="host", KSPIDER_CLASSIFY_BATCH_BYTES="4096", KSPIDER_VERBOSE="1")
    done = subprocess.run([exe, str(world["reads"]), str(K), str(SCALED), str(world["db"]), prefix, "2", "--min-hits", "2"], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert "classify:" in done.stdout and "on the host" in done.stdout and "hit words" in done.stdout
    assert (open(prefix + "_kSpider_classify.tsv").read(), open(prefix + "_kSpider_classify_hits.tsv").read()) == _want(world, 2)
    assert subprocess.run([exe, str(world["reads"]), str(K)], capture_output=True).returncode == 2
    bad = subprocess.run([exe, str(world["reads"]), str(K), "0", str(world["db"]), prefix, "1"], env=env, capture_output=True, text=True)
    assert bad.returncode == 1 and "scaled" in bad.stderr


def test_the_python_module_in_host_mode(world, monkeypatch):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "kspider_amd", "lib"))
    try:
        import _kSpider_internal as ks
    finally:
        sys.path.pop(0)
    monkeypatch.setenv("KSPIDER_CLASSIFY", "host")
    prefix = str(world["dir"] / "pyext")
    ks.classify(input=str(world["reads"]), kSize=K, scaled=SCALED, db=str(world["db"]), out_prefix=prefix, user_threads=2, min_hits=2)
    assert (open(prefix + "_kSpider_classify.tsv").read(), open(prefix + "_kSpider_classify_hits.tsv").read()) == _want(world, 2)
    with pytest.raises(RuntimeError) as ei:
        ks.classify(str(world["reads"]), K, 0, str(world["db"]), prefix)
    assert "scaled" in str(ei.value)


def test_refusals_write_nothing(world, monkeypatch):
    monkeypatch.setenv("KSPIDER_CLASSIFY", "host")
    prefix = str(world["dir"] / "refused")

    def refuse(code, *args, **env):
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        with pytest.raises(engine.KspError) as ei:
            engine.classify_files(*args)
        for name in env:
            monkeypatch.delenv(name)
        assert ei.value.code == code, str(ei.value)
        assert not os.path.exists(prefix + "_kSpider_classify.tsv") and not os.path.exists(prefix + "_kSpider_classify_hits.tsv")
        return str(ei.value)

    reads, db = str(world["reads"]), str(world["db"])
    refuse(engine.KSP_E_ARG, reads, 0, SCALED, db, prefix)
    refuse(engine.KSP_E_ARG, reads, 65, SCALED, db, prefix)
    refuse(engine.KSP_E_ARG, reads, K, 0, db, prefix)
    assert "min_hits" in refuse(engine.KSP_E_ARG, reads, K, SCALED, db, prefix, 1, 0)
    refuse(engine.KSP_E_ARG, reads, K, SCALED, db, "")
    assert "BATCH_BYTES" in refuse(engine.KSP_E_ARG, reads, K, SCALED, db, prefix, KSPIDER_CLASSIFY_BATCH_BYTES="1023")
    assert "host" in refuse(engine.KSP_E_ARG, reads, K, SCALED, db, prefix, KSPIDER_CLASSIFY="gpu")
    monkeypatch.setenv("KSPIDER_CLASSIFY", "host")
    refuse(engine.KSP_E_IO, str(world["dir"] / "nope.fa"), K, SCALED, db, prefix)
    refuse(engine.KSP_E_IO, reads, K, SCALED, str(world["dir"] / "nope.pack"), prefix)
    refuse(engine.KSP_E_IO, reads, 25, SCALED, db, prefix)   # no signature of that ksize
    pack = str(world["dir"] / "k.pack")
    engine.pack(db, K, pack, 1)
    assert "packed with kSize" in refuse(engine.KSP_E_ARG, reads, 31, SCALED, pack, prefix)

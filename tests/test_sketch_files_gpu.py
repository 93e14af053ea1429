"""The file driver of the sketcher on the device (kspider_sketch, csrc/sketch_files.cpp over ksp_sketch_host): a directory of
FASTA / FASTQ / gz files gives the bytes host mode gives, at the default batch and at 4 KiB batches, and kspider_pairwise_sigs on
the signatures writes the table the oracle writes for the restated sketches."""
import os

import numpy as np
import pytest

import sketch_restate as R
from kspider_amd import engine
from test_sketch_files_cpu import K, SCALED, _seq_of, genomes  # noqa: F401  (the module's directory of inputs)

pytestmark = pytest.mark.gpu


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_device_writes_the_bytes_of_host_mode(monkeypatch, genomes, tmp_path):
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    engine.sketch_files(genomes[0], K, SCALED, str(tmp_path / "host"), 2)
    want = _files(tmp_path / "host")
    assert len(want) == len(genomes[1])
    monkeypatch.delenv("KSPIDER_SKETCH")
    engine.sketch_files(genomes[0], K, SCALED, str(tmp_path / "device"), 2)
    assert _files(tmp_path / "device") == want
    monkeypatch.setenv("KSPIDER_SKETCH_BATCH_BYTES", "4096")
    engine.sketch_files(genomes[0], K, SCALED, str(tmp_path / "small"), 3)
    assert _files(tmp_path / "small") == want
    monkeypatch.setenv("KSPIDER_SKETCH", "device")
    monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", "2")
    engine.sketch_files(genomes[0], K, SCALED, str(tmp_path / "two"), 1)
    assert _files(tmp_path / "two") == want


def test_pairwise_on_the_signatures_matches_the_oracle(monkeypatch, oracle_lib, genomes, tmp_path):
    monkeypatch.delenv("KSPIDER_SKETCH", raising=False)
    sigs = tmp_path / "sigs"
    engine.sketch_files(genomes[0], K, SCALED, str(sigs), 2)
    prefix = str(tmp_path / "out")
    engine.pairwise_sigs(str(sigs), K, prefix, 2)
    # the restated sketches in the order of the names (glob order = sorted)
    mh = R.max_hash_of(SCALED)
    runs = []
    for name in sorted(genomes[1]):
        seq = _seq_of(genomes[1][name][0])
        runs.append(R.sketch(seq, [0, len(seq)], K, mh)[0])
    keys, off = R.flat(runs)
    oprefix = str(tmp_path / "orc")
    oracle_lib.index_from_sketches(oprefix, keys, off)
    oracle_lib.ref_pairwise(oprefix, 1)
    assert open(prefix + "_kSpider_pairwise.tsv", "rb").read() == open(oprefix + "_kSpider_pairwise.tsv", "rb").read()
    assert open(prefix + ".namesMap").read().split()[:3] == [str(len(runs)), "1", "g1"]

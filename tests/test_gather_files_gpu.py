"""The file entry of gather on the GPU (kspider_gather, kspider_amd/csrc/sketch_pack.cpp) and its executable (lib/gather): the TSV
over a small .sig directory and over its pack, byte for byte against one written here from the restatement's rows and
engine.format_float; a failing call leaves no file."""
import json
import os
import subprocess

import numpy as np
import pytest

import gather_restate as GR
from kspider_amd import engine

pytestmark = pytest.mark.gpu
N_DB, N_Q, KSIZE, MIN_HASHES = 12, 3, 31, 4
HEADER = "query\trank\tmatch\toverlap\tunique\tf_orig_query\tf_unique_to_query\tf_match\tremaining\n"
TOOL = os.path.join(os.path.dirname(engine.LIB_PATH), "gather")


def _write_sig(path, ksize, mins):
    with open(path, "w") as f:
        f.write(json.dumps([{"signatures": [{"ksize": ksize, "mins": [int(m) for m in mins]}]}]))


@pytest.fixture(scope="module")
def sig_dirs(tmp_path_factory):
    """(root, the database's runs, the queries' runs, the names of both sides): source 4 of the database lacks the ksize"""
    root = tmp_path_factory.mktemp("gather_sigs")
    rng = np.random.default_rng(77)
    (root / "db").mkdir()
    (root / "q").mkdir()
    db, q, db_names, q_names = [], [], [], []
    for i in range(N_DB):
        run = np.sort(rng.choice(500, size=40 + 5 * i, replace=False)).astype(np.uint64)
        _write_sig(str(root / "db" / f"genome{i:02d}.sig"), 21 if i == 4 else KSIZE, run)
        if i != 4:
            db.append(run)
            db_names.append(f"genome{i:02d}")
    for j in range(N_Q):
        run = np.unique(np.concatenate([rng.choice(db[3 * j + k], size=20, replace=False) for k in range(3)] + [np.arange(10**6, 10**6 + 7 + j)])).astype(np.uint64)
        _write_sig(str(root / "q" / f"sample{j}.sig"), KSIZE, run)
        q.append(run)
        q_names.append(f"sample{j}")
    return root, db, q, db_names, q_names


def _expected(db, q, db_names, q_names, max_matches=0):
    text = HEADER
    for query, rank, source, overlap, unique, remaining in GR.gather(db, q, MIN_HASHES, max_matches):
        floats = [np.float32(overlap) / np.float32(len(q[query])), np.float32(unique) / np.float32(len(q[query])), np.float32(overlap) / np.float32(len(db[source]))]
        text += "\t".join([q_names[query], str(rank), db_names[source], str(overlap), str(unique)] + [engine.format_float(float(v)) for v in floats] + [str(remaining)]) + "\n"
    return text.encode()


def test_directory_pack_and_executable_write_the_same_file(sig_dirs):
    root, db, q, db_names, q_names = sig_dirs
    want = _expected(db, q, db_names, q_names)
    assert want.count(b"\n") > 1 + 2 * N_Q
    engine.pack(str(root / "db"), KSIZE, str(root / "db.kspack"), 2)
    engine.pack(str(root / "q"), KSIZE, str(root / "q.kspack"), 2)
    for n, (d, s) in enumerate([("db", "q"), ("db.kspack", "q"), ("db", "q.kspack"), ("db.kspack", "q.kspack")]):
        out = str(root / f"OUT{n}")
        engine.gather(str(root / d), str(root / s), KSIZE, out, 2, min_hashes=MIN_HASHES)
        assert open(out + "_kSpider_gather.tsv", "rb").read() == want
    out = str(root / "TOOL")
    done = subprocess.run([TOOL, str(root / "db.kspack"), str(root / "q"), str(KSIZE), out, "2", str(MIN_HASHES)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert open(out + "_kSpider_gather.tsv", "rb").read() == want
    done = subprocess.run([TOOL, str(root / "db"), str(root / "q.kspack"), str(KSIZE), out + "1", "2", str(MIN_HASHES), "--max-matches", "1"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert open(out + "1_kSpider_gather.tsv", "rb").read() == _expected(db, q, db_names, q_names, max_matches=1)
    assert not [f for f in os.listdir(root) if f.endswith(".partial")]


def test_a_failing_call_leaves_no_file(sig_dirs, monkeypatch):
    root, *_ = sig_dirs
    (root / "empty").mkdir(exist_ok=True)
    for kwargs, code in [(dict(min_hashes=0), engine.KSP_E_ARG), (dict(min_hashes=1, kSize=21, db="db.kspack"), engine.KSP_E_ARG)]:
        out = str(root / "NO")
        with pytest.raises(engine.KspError) as ei:
            engine.gather(str(root / kwargs.get("db", "db")), str(root / "q"), kwargs.get("kSize", KSIZE), out, 2, min_hashes=kwargs["min_hashes"])
        assert ei.value.code == code and not os.path.exists(out + "_kSpider_gather.tsv")
    monkeypatch.setenv("KSPIDER_DEVICE", "99")                                     # the inputs load, the device call fails
    out = str(root / "NODEVICE")
    with pytest.raises(engine.KspError) as ei:
        engine.gather(str(root / "db"), str(root / "q"), KSIZE, out, 2, min_hashes=MIN_HASHES)
    assert ei.value.code == engine.KSP_E_HIP and "no such device" in str(ei.value)
    assert not os.path.exists(out + "_kSpider_gather.tsv") and not os.path.exists(out + "_kSpider_gather.tsv.partial")
    done = subprocess.run([TOOL, str(root / "db"), str(root / "q"), str(KSIZE), out, "2", "0"], capture_output=True, text=True)
    assert done.returncode == 1 and "min_hashes" in done.stderr and not os.path.exists(out + "_kSpider_gather.tsv")
    assert subprocess.run([TOOL, str(root / "db")], capture_output=True).returncode == 2

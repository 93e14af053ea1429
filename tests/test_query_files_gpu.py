"""The file entry of query mode on the GPU (kspider_query, kspider_amd/csrc/sketch_pack.cpp): its three files against those of a
pairwise run over one merged directory (database names glob first), byte for byte; a pack file in place of the directory; a
.sig database with a signature that lacks the ksize and a bare .gz name; and kspider_topk over the result."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest

import oracle
import query_inputs as Q
from kspider_amd import engine

pytestmark = pytest.mark.gpu
SUFFIXES = (".namesMap", "_kSpider_seqToKmersNo.tsv", "_kSpider_pairwise.tsv")
N_DB, N_Q = 30, 6


def _read(prefix):
    return [open(prefix + s, "rb").read() for s in SUFFIXES]


def _rows_of_mode(tsv, n_names_db, mode):
    """The header and the rows of a pairwise TSV over the union that the mode keeps (ids are 1-based)."""
    lines = tsv.split(b"\n")
    keep = [lines[0]]
    for line in lines[1:]:
        if not line:
            continue
        a, b = (int(x) for x in line.split(b"\t")[:2])
        if b > n_names_db and (mode == Q.CROSS_AND_SELF or a <= n_names_db):
            keep.append(line)
    return b"\n".join(keep) + b"\n"


@pytest.fixture(scope="module")
def runs():
    rng = np.random.default_rng(2024)
    return [np.sort(rng.choice(600, size=50 + 3 * i, replace=False)).astype(np.uint64) for i in range(N_DB + N_Q)]


@pytest.fixture(scope="module")
def bin_dirs(runs, tmp_path_factory):
    root = tmp_path_factory.mktemp("bins")
    for d in ("db", "q", "merged"):
        (root / d).mkdir()
    for i, r in enumerate(runs):   # "a..." globs before "z...": the merged directory lists the database first
        name = f"a_db{i:03d}.bin" if i < N_DB else f"z_query{i - N_DB:03d}.bin"
        oracle.write_bin_sketch(str(root / ("db" if i < N_DB else "q") / name), r, slot_seed=7 + i)
        shutil.copy(str(root / ("db" if i < N_DB else "q") / name), str(root / "merged" / name))
    engine.pairwise_bins(str(root / "merged"), str(root / "MERGED"), 2)
    return root, _read(str(root / "MERGED"))


@pytest.mark.parametrize("mode", [Q.CROSS_AND_SELF, Q.CROSS])
def test_directories_against_the_merged_run(bin_dirs, mode):
    root, merged = bin_dirs
    out = str(root / f"OUT{mode}")
    engine.query(str(root / "db"), str(root / "q"), 0, out, 2, mode=mode)
    got = _read(out)
    assert got[0] == merged[0] and got[1] == merged[1]
    assert got[2] == _rows_of_mode(merged[2], N_DB, mode) and got[2].count(b"\n") > 1 + N_Q
    assert not [f for f in os.listdir(root) if f.endswith(".partial")]


@pytest.mark.parametrize("mode", [Q.CROSS_AND_SELF, Q.CROSS])
def test_pack_file_in_place_of_the_directory(bin_dirs, mode):
    root, merged = bin_dirs
    engine.pack(str(root / "db"), 0, str(root / "db.kspack"), 2)
    engine.pack(str(root / "q"), 0, str(root / "q.kspack"), 2)
    for db, q in [("db.kspack", "q"), ("db", "q.kspack"), ("db.kspack", "q.kspack")]:
        out = str(root / f"PACKED{mode}")
        engine.query(str(root / db), str(root / q), 0, out, 2, mode=mode)
        got = _read(out)
        assert got[:2] == merged[:2] and got[2] == _rows_of_mode(merged[2], N_DB, mode)


def _write_sig(path, ksize, mins, compress=False):
    text = json.dumps([{"signatures": [{"ksize": ksize, "mins": [int(m) for m in mins]}]}])
    with (gzip.open(path, "wt") if compress else open(path, "w")) as f:
        f.write(text)


@pytest.mark.parametrize("mode", [Q.CROSS_AND_SELF, Q.CROSS])
def test_signature_database(runs, tmp_path, mode):
    for d in ("db", "q", "merged"):
        (tmp_path / d).mkdir()
    n_names = 0
    for i, r in enumerate(runs[:12] + runs[N_DB:]):
        side = "db" if i < 12 else "q"
        name = f"a_db{i:03d}.sig" if i < 12 else f"z_query{i:03d}.sig"
        _write_sig(str(tmp_path / side / name), 21 if i == 4 else 31, r, compress=(i % 5 == 0))   # source 4 lacks ksize 31
        shutil.copy(str(tmp_path / side / name), str(tmp_path / "merged" / name))
        n_names += side == "db"
    for d in ("db", "merged"):
        (tmp_path / d / "a_db900.gz").write_bytes(b"")            # a bare .gz name: a group without a sketch
    n_names += 1
    engine.pairwise_sigs(str(tmp_path / "merged"), 31, str(tmp_path / "MERGED"), 2)
    merged = _read(str(tmp_path / "MERGED"))
    engine.pack(str(tmp_path / "db"), 31, str(tmp_path / "db.kspack"), 2)
    for db in ("db", "db.kspack"):
        out = str(tmp_path / "OUT")
        engine.query(str(tmp_path / db), str(tmp_path / "q"), 31, out, 2, mode=mode)
        got = _read(out)
        assert got[:2] == merged[:2] and got[2] == _rows_of_mode(merged[2], n_names, mode)
    assert merged[0].startswith(b"%d\n" % (n_names + N_Q)) and b"\t5\t" not in merged[1]   # the names count both; group 5 has no k-mers row
    with pytest.raises(engine.KspError) as ei:                     # the pack was made for ksize 31
        engine.query(str(tmp_path / "db.kspack"), str(tmp_path / "q"), 21, str(tmp_path / "NO"), 2, mode=mode)
    assert ei.value.code == engine.KSP_E_ARG and not os.path.exists(str(tmp_path / "NO.namesMap"))


def test_topk_over_the_result(bin_dirs, runs):
    root, _ = bin_dirs
    out = str(root / "TOPK")
    engine.query(str(root / "db"), str(root / "q"), 0, out, 2, mode=Q.CROSS)
    engine.topk(out, "max_cont", 3)
    first = {}
    for line in open(out + "_kSpider_topk_max_cont.tsv").read().splitlines()[1:]:
        source, hit, neighbour, _ = line.split("\t")
        if hit == "1":
            first[source] = neighbour
    sizes = [np.float32(r.size) for r in runs]
    for j in range(N_Q):   # the best database hit by brute force, in the writer's single-precision maths
        shared = [np.float32(np.intersect1d(runs[i], runs[N_DB + j]).size) for i in range(N_DB)]
        value = [max(shared[i] / sizes[i], shared[i] / sizes[N_DB + j]) for i in range(N_DB)]
        best = {f"a_db{i:03d}" for i in range(N_DB) if value[i] == max(value)}
        assert max(value) > 0 and first[f"z_query{j:03d}"] in best

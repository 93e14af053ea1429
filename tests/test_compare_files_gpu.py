"""The file path of compare on the GPU, end to end: counted signatures written by the sketch driver in host mode (--abund) and by
hand — a flat one, one that lists a hash twice, one that shares nothing —, then kspider_compare and the `compare` executable
(kspider_amd/csrc/sketch_pack.cpp).  The TSV's integer columns equal the restatement's (tests/compare_restate.py); its doubles are
within 2e-6 (all four lie in [0, 1]: "%.6g" rounds at no more than 5e-7 on each side, the rest is slack for the last bits of acos);
the matrix repeats the TSV's text; --against writes the database x sample rows only; a refused call leaves no file."""
import json
import os
import random
import subprocess

import pytest

import compare_restate as R
import sketch_inputs as I
from kspider_amd import engine

pytestmark = pytest.mark.gpu
K, SCALED = 21, 2
LIB = os.path.dirname(engine.LIB_PATH)
HEADER = "source_1\tsource_2\tshared_kmers\tdot\tmass_1\tmass_2\tcosine\tangular_similarity\tweighted_containment_1\tweighted_containment_2"
TOL = 2e-6


def _fasta(records):
    return "".join(">" + name + "\n" + seq + "\n" for name, seq in records)


def _sig(path, mins, abunds=None):
    sig = {"ksize": K, "mins": [int(m) for m in mins]}
    if abunds is not None:
        sig["abundances"] = [int(a) for a in abunds]
    path.write_text(json.dumps([{"class": "sourmash_signature", "signatures": [sig]}]))


def _read(sig_dir):
    """name -> {hash: abundance} of a directory of signatures as the loader hands them on: a flat one is all ones, a hash listed
    twice has its abundances added"""
    out = {}
    for f in sorted(os.listdir(sig_dir)):
        sig = json.load(open(os.path.join(sig_dir, f)))[0]["signatures"][0]
        src = {}
        for m, a in zip(sig["mins"], sig.get("abundances", [1] * len(sig["mins"]))):
            src[m] = src.get(m, 0) + a
        out[f[:-len(".sig")]] = src
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(root, samples by name, database by name): three genomes of 1 500 bases; sample a = reads of g0 at depth 6 and of g1 at 2,
    b = g0 at 3 and g2 at 4, c = a's file again; by hand: flat (every other hash of a, no abundances), twice (a hash listed twice),
    lonely (hashes nobody else has)."""
    root = tmp_path_factory.mktemp("compare")
    rng = random.Random(19)
    genomes = {f"g{i}": I.bases(rng, 1500) for i in range(3)}

    def reads(depths):
        out = []
        for g, depth in depths.items():
            for _ in range(depth * 15):
                at = rng.randrange(1400)
                out.append(genomes[g][at:at + 100])
        rng.shuffle(out)
        return [(f"r{i}", r) for i, r in enumerate(out)]

    samples = {"a": reads({"g0": 6, "g1": 2}), "b": reads({"g0": 3, "g2": 4})}
    samples["c"] = samples["a"]
    for d in ("genomes", "reads"):
        (root / d).mkdir()
    for name, text in genomes.items():
        (root / "genomes" / (name + ".fa")).write_text(_fasta([(name, text)]))
    for name, recs in samples.items():
        (root / "reads" / (name + ".fa")).write_text(_fasta(recs))
    old = os.environ.get("KSPIDER_SKETCH")
    os.environ["KSPIDER_SKETCH"] = "host"
    try:
        engine.sketch_files(str(root / "reads"), K, SCALED, str(root / "samples"), 2, abund=True)
        engine.sketch_files(str(root / "genomes"), K, SCALED, str(root / "db"), 2)
    finally:
        if old is None:
            del os.environ["KSPIDER_SKETCH"]
        else:
            os.environ["KSPIDER_SKETCH"] = old
    a = json.load(open(root / "samples" / "a.sig"))[0]["signatures"][0]
    assert max(a["abundances"]) > 3 and len(a["mins"]) > 500
    _sig(root / "samples" / "flat.sig", a["mins"][::2])
    _sig(root / "samples" / "twice.sig", [a["mins"][0], a["mins"][5], a["mins"][0], 12345], [4, 2, 9, 1])
    _sig(root / "samples" / "lonely.sig", [3, 5, 7], [1, 2, 3])
    return root, _read(root / "samples"), _read(root / "db")


def _names(prefix):
    lines = open(prefix + ".namesMap").read().splitlines()
    ids = {}
    for ln in lines[1:]:
        i, name = ln.split(" ", 1)
        ids[int(i)] = name
    assert int(lines[0]) == len(ids)
    return ids


def _check_tsv(prefix, db, samples, mode):
    """the TSV against the restatement over the sources in id order; -> {(id_1, id_2): the text of the angular column}"""
    ids = _names(prefix)
    order = [ids[i] for i in sorted(ids)]
    assert order == sorted(db) + sorted(samples)
    sources = [db[n] for n in sorted(db)] + [samples[n] for n in sorted(samples)]
    total, sq = R.totals(sources)
    want = R.rows(sources[:len(db)], sources[len(db):], mode)
    lines = open(prefix + "_kSpider_compare.tsv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + len(want)
    angular = {}
    for ln, row in zip(lines[1:], want):
        cols = ln.split("\t")
        assert [int(c) for c in cols[:6]] == [row[0] + 1, row[1] + 1, *row[2:]]
        vals = R.values(row, total[row[0]], sq[row[0]], total[row[1]], sq[row[1]])
        assert all(abs(float(c) - v) <= TOL and 0.0 <= float(c) <= 1.0 for c, v in zip(cols[6:], vals)), (ln, vals)
        angular[(row[0] + 1, row[1] + 1)] = cols[7]
    kmers = open(prefix + "_kSpider_seqToKmersNo.tsv").read().splitlines()
    assert kmers[0] == "ID\tseq\tkmers" and [int(ln.split("\t")[1]) for ln in kmers[1:]] == sorted(ids)
    return angular, want


def _outputs(root, tag):
    return sorted(f for f in os.listdir(root) if f.startswith(tag))


def test_all_pairs_with_the_matrix_and_the_executable(world):
    root, samples, _ = world
    out = str(root / "ALL")
    engine.compare(str(root / "samples"), K, out, 2, matrix=True)
    angular, want = _check_tsv(out, {}, samples, R.CROSS_AND_SELF)
    names = sorted(samples)
    at = {n: i + 1 for i, n in enumerate(names)}
    assert angular[(at["a"], at["c"])] == "1"                                   # one sample twice: exactly 1
    assert not [p for p in angular if at["lonely"] in p]                        # shares nothing: no row
    assert (at["a"], at["flat"]) in angular and (at["a"], at["twice"]) in angular
    twice = [r for r in want if (r[0] + 1, r[1] + 1) == (at["a"], at["twice"])][0]
    assert twice[2] == 2 and twice[5] == 13 + 2                                 # the hash listed twice holds 4 + 9
    csv = open(out + "_kSpider_compare_matrix.csv").read().splitlines()
    assert csv[0] == ",".join(names) and len(csv) == 1 + len(names)
    cells = [ln.split(",") for ln in csv[1:]]
    for i in range(len(names)):
        assert len(cells[i]) == len(names) and cells[i][i] == "1"
        for j in range(i + 1, len(names)):
            assert cells[i][j] == cells[j][i] == angular.get((i + 1, j + 1), "0")
    # the executable writes the same bytes
    tool = str(root / "ALLTOOL")
    done = subprocess.run([os.path.join(LIB, "compare"), str(root / "samples"), str(K), tool, "2", "--matrix"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    for suffix in (".namesMap", "_kSpider_seqToKmersNo.tsv", "_kSpider_compare.tsv", "_kSpider_compare_matrix.csv"):
        assert open(tool + suffix, "rb").read() == open(out + suffix, "rb").read(), suffix
    assert _outputs(root, "ALLTOOL") == sorted("ALLTOOL" + s for s in (".namesMap", "_kSpider_seqToKmersNo.tsv", "_kSpider_compare.tsv", "_kSpider_compare_matrix.csv"))


def test_against_a_database_directory_and_a_pack(world):
    root, samples, db = world
    out = str(root / "DB")
    engine.compare(str(root / "samples"), K, out, 2, against=str(root / "db"))
    angular, want = _check_tsv(out, db, samples, R.CROSS)
    assert want and all(r[0] < len(db) <= r[1] for r in want) and not os.path.exists(out + "_kSpider_compare_matrix.csv")
    assert all(r[3] == r[5] and r[4] == r[2] for r in want)                     # a flat database: dot = the sample's mass on the shared hashes
    engine.pack(str(root / "db"), K, str(root / "db.pack"), 2)
    done = subprocess.run([os.path.join(LIB, "compare"), str(root / "samples"), str(K), out + "PACK", "2", "--against", str(root / "db.pack")],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert open(out + "PACK_kSpider_compare.tsv", "rb").read() == open(out + "_kSpider_compare.tsv", "rb").read()


def test_a_refused_call_leaves_no_file(world, tmp_path):
    root, _, _ = world
    bad = tmp_path / "bad"
    bad.mkdir()
    _sig(bad / "fine.sig", [1, 2, 3], [1, 1, 1])
    _sig(bad / "zero.sig", [2, 3, 4], [5, 0, 5])
    with pytest.raises(engine.KspError) as ei:
        engine.compare(str(bad), K, str(tmp_path / "OUT"), 2, matrix=True)
    assert ei.value.code == engine.KSP_E_ARG and "query source 1 has an abundance of 0" in str(ei.value)
    done = subprocess.run([os.path.join(LIB, "compare"), str(bad), str(K), str(tmp_path / "TOOL"), "2"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 1 and "abundance of 0" in done.stderr
    done = subprocess.run([os.path.join(LIB, "compare"), str(root / "samples"), str(K), str(tmp_path / "TOOL"), "2", "--against", str(root / "db"), "--matrix"],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 1 and "matrix" in done.stderr
    assert subprocess.run([os.path.join(LIB, "compare"), str(bad), str(K)], capture_output=True, timeout=120).returncode == 2
    assert sorted(os.listdir(tmp_path)) == ["bad"]

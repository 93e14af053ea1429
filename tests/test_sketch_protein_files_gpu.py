"""The file driver with the molecule flags on the device (kspider_sketch over ksp_sketch_host_mol): a small .faa directory and a
translated genome directory give the bytes host mode gives, at two batch sizes; then kspider_pack and kspider_query at 3k over
those signatures give the shared hashes and containments that the restatement predicts."""
import os
import shutil

import pytest

import sketch_protein_restate as P
from kspider_amd import engine
from test_sketch_protein_cpu import _seq_of, inputs  # noqa: F401  (the module's directories of inputs)

pytestmark = pytest.mark.gpu


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _device_equals_host(monkeypatch, src, k, scaled, tmp_path, **kw):
    monkeypatch.delenv("KSPIDER_SKETCH_BATCH_BYTES", raising=False)
    monkeypatch.setenv("KSPIDER_SKETCH", "host")
    engine.sketch_files(src, k, scaled, str(tmp_path / "host"), 2, **kw)
    want = _files(tmp_path / "host")
    monkeypatch.delenv("KSPIDER_SKETCH")
    engine.sketch_files(src, k, scaled, str(tmp_path / "device"), 2, **kw)
    assert _files(tmp_path / "device") == want and len(want) == 3
    monkeypatch.setenv("KSPIDER_SKETCH_BATCH_BYTES", "1024")
    engine.sketch_files(src, k, scaled, str(tmp_path / "small"), 3, **kw)
    assert _files(tmp_path / "small") == want
    monkeypatch.delenv("KSPIDER_SKETCH_BATCH_BYTES")
    return tmp_path / "device"


def _query_matches(sigs, names, records_of, k, scaled, mol, translated, tmp_path):
    """The last name is the query, the others the database; rows of the TSV against the restated sketches.  The containments are
    printed with six significant digits: 1e-5 relative covers that and the float division."""
    (tmp_path / "q").mkdir()
    shutil.move(str(sigs / (names[-1] + ".sig")), str(tmp_path / "q" / (names[-1] + ".sig")))
    engine.pack(str(sigs), 3 * k, str(tmp_path / "db.kspack"), 2)
    out = str(tmp_path / "OUT")
    engine.query(str(tmp_path / "db.kspack"), str(tmp_path / "q"), 3 * k, out, 2)
    assert open(out + ".namesMap").read().split() == [str(len(names))] + [x for i, n in enumerate(names) for x in (str(i + 1), n)]
    sets = []
    for n in names:
        seq = _seq_of(records_of[n])
        sets.append(set(P.counted_sketch(seq, [0, len(seq)], k, mol, translated, P.max_hash_of(scaled))[0]))
    want = {}
    for i in range(len(names) - 1):
        shared = len(sets[i] & sets[-1])
        if shared:
            want[(i + 1, len(names))] = (shared, shared / max(len(sets[i]), len(sets[-1])), shared / min(len(sets[i]), len(sets[-1])))
    rows = [line.split("\t") for line in open(out + "_kSpider_pairwise.tsv").read().splitlines()[1:]]
    got = {(int(r[0]), int(r[1])): (int(r[2]), float(r[3]), float(r[5])) for r in rows}
    assert sorted(got) == sorted(want) and len(want) >= 1
    for pair, (shared, lo, hi) in want.items():
        assert got[pair][0] == shared and got[pair][1] == pytest.approx(lo, rel=1e-5) and got[pair][2] == pytest.approx(hi, rel=1e-5)


@pytest.mark.parametrize("mol", [P.PROTEIN, P.DAYHOFF])
def test_a_directory_of_proteomes(monkeypatch, inputs, tmp_path, mol):
    sigs = _device_equals_host(monkeypatch, inputs[2], 7, 3, tmp_path, moltype=mol, abund=True)
    _query_matches(sigs, ["p1", "p2", "p3"], inputs[3], 7, 3, mol, False, tmp_path)


@pytest.mark.parametrize("mol", [P.PROTEIN, P.HP])
def test_a_translated_directory_of_genomes(monkeypatch, inputs, tmp_path, mol):
    sigs = _device_equals_host(monkeypatch, inputs[0], 10, 2, tmp_path, moltype=mol, translate=True, abund=True)
    _query_matches(sigs, ["g1", "g2", "g3"], inputs[1], 10, 2, mol, True, tmp_path)

"""The use DESIGN.md 7r is written for, end to end on the device: proteins against translated genomes.  Three genomes that each
carry two planted genes (one on each strand, in frames 1 and 2) are sketched with translate, the six proteins as protein input;
`pack` + `query` at ksize 3k find every protein whole in its genome, and `gather` and the abundance-weighted gather decompose the
translated genomes into the proteins.  Every expected row comes from the restatement (tests/sketch_protein_restate.py) through
gather_restate / gather_abund_restate; the gather files are written by the helpers of tests/test_gather_files_gpu.py and
tests/test_gather_abund_files_gpu.py and compared byte for byte."""
import random

import pytest

import sketch_inputs as DI
import sketch_protein_inputs as I
import sketch_protein_restate as P
from kspider_amd import engine
from test_gather_abund_files_gpu import _tsv as _weighted_tsv
from test_gather_files_gpu import MIN_HASHES, _expected as _gather_tsv
from test_sketch_protein_cpu import _fasta, _seq_of

pytestmark = pytest.mark.gpu
K, SCALED = 7, 3
GENOMES = ["g1", "g2", "g3"]
PROTEINS = ["p1f", "p1r", "p2f", "p2r", "p3f", "p3r"]      # p<n>f lies on the forward strand of g<n>, p<n>r on its reverse strand


def _back_translation(rng, protein):
    """Bases that translate to the protein: any of its codons for every residue."""
    codons = {}
    for i, aa in enumerate(P.GENETIC_CODE):
        codons.setdefault(aa, []).append("TCAG"[i // 16] + "TCAG"[i // 4 % 4] + "TCAG"[i % 4])
    return "".join(rng.choice(codons[aa]) for aa in protein)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """(root, the genomes' records, the proteins' records): g<n>.fa is one record of 6 000 random bases wrapped at 60 columns in
    which the back-translation of p<n>f lies at an offset = 1 mod 3 and the reverse complement of the back-translation of p<n>r at
    an offset = 2 mod 3; a protein is 249 random residues and a '*'."""
    root = tmp_path_factory.mktemp("planted_genes")
    rng = random.Random(90)
    (root / "genomes").mkdir()
    (root / "proteins").mkdir()
    genomes, proteins = {}, {}
    for g in GENOMES:
        text = DI.bases(rng, 6000, lower=0.1)
        fw, rv = I.residues(rng, 249) + "*", I.residues(rng, 249) + "*"
        at_f, at_r = 3 * rng.randrange(100, 600) + 1, 3 * rng.randrange(1000, 1600) + 2
        gene_f, gene_r = _back_translation(rng, fw), P.revcomp(_back_translation(rng, rv))
        assert P.translate(gene_f) == fw and P.translate(P.revcomp(gene_r)) == rv and at_f + 750 <= at_r
        text = text[:at_f] + gene_f + text[at_f + 750:at_r] + gene_r + text[at_r + 750:]
        assert len(text) == 6000
        genomes[g] = [(g, text)]
        proteins[g.replace("g", "p") + "f"], proteins[g.replace("g", "p") + "r"] = [("forward", fw)], [("reverse", rv)]
        (root / "genomes" / (g + ".fa")).write_text(_fasta(genomes[g]))
    for p, records in proteins.items():
        (root / "proteins" / (p + ".faa")).write_text(_fasta(records))
    return root, genomes, proteins


_made = {}


def _sketched(planted, mol):
    """One molecule type's (genome signatures, protein signatures, {genome: {hash: count}}, {protein: {hash: count}}): the
    directories made on the device, the dicts by the restatement, both once."""
    root, genomes, proteins = planted
    if mol not in _made:
        g_sigs, p_sigs = root / f"g_sigs{mol}", root / f"p_sigs{mol}"
        engine.sketch_files(str(root / "genomes"), K, SCALED, str(g_sigs), 2, moltype=mol, translate=True, abund=True)
        engine.sketch_files(str(root / "proteins"), K, SCALED, str(p_sigs), 2, moltype=mol, abund=True)
        mh = P.max_hash_of(SCALED)
        one = lambda records, translated: P.counted_sketch(_seq_of(records), [0, len(_seq_of(records))], K, mol, translated, mh)[0]   # noqa: E731
        _made[mol] = (g_sigs, p_sigs, {g: one(genomes[g], True) for g in GENOMES}, {p: one(proteins[p], False) for p in PROTEINS})
    return _made[mol]


@pytest.mark.parametrize("mol", [P.PROTEIN, P.DAYHOFF])
def test_proteins_inside_translated_genomes(monkeypatch, planted, mol):
    monkeypatch.delenv("KSPIDER_SKETCH", raising=False)
    root = planted[0]
    g_sigs, p_sigs, G, Pr = _sketched(planted, mol)
    for name, want in list(G.items()) + list(Pr.items()):          # the signatures themselves are the restated sketches
        mins, abunds = engine.sig_read(str((g_sigs if name in G else p_sigs) / (name + ".sig")), 3 * K)
        assert mins.tolist() == sorted(want) and abunds.tolist() == [want[h] for h in sorted(want)] and len(want) > 0
    engine.pack(str(g_sigs), 3 * K, str(root / f"genomes{mol}.kspack"), 2)
    out = str(root / f"QUERY{mol}")
    engine.query(str(root / f"genomes{mol}.kspack"), str(p_sigs), 3 * K, out, 2)
    names = GENOMES + PROTEINS
    assert open(out + ".namesMap").read().split() == [str(len(names))] + [x for i, n in enumerate(names) for x in (str(i + 1), n)]
    want = {}
    for i, g in enumerate(GENOMES):
        for j, p in enumerate(PROTEINS):
            shared = len(set(G[g]) & set(Pr[p]))
            if shared:
                want[(i + 1, len(GENOMES) + j + 1)] = (shared, shared / max(len(G[g]), len(Pr[p])), shared / min(len(G[g]), len(Pr[p])))
    rows = [line.split("\t") for line in open(out + "_kSpider_pairwise.tsv").read().splitlines()[1:]]
    got = {(int(r[0]), int(r[1])): r[2:] for r in rows}
    assert sorted(got) == sorted(want) and len(got) == len(rows)   # no row for a pair whose restated sketches share nothing
    for pair, (shared, lo, hi) in want.items():   # (six significant digits are printed: 1e-5 relative covers that and the float division)
        assert int(got[pair][0]) == shared and float(got[pair][1]) == pytest.approx(lo, rel=1e-5) and float(got[pair][3]) == pytest.approx(hi, rel=1e-5)
    for j, p in enumerate(PROTEINS):               # every protein lies whole in its genome, on either strand
        i = GENOMES.index("g" + p[1])
        row = got[(i + 1, len(GENOMES) + j + 1)]
        assert int(row[0]) == len(Pr[p]) > 0 and set(Pr[p]) <= set(G[GENOMES[i]])
        assert row[3] == "1" == engine.format_float(1.0)


@pytest.mark.parametrize("mol", [P.PROTEIN, P.DAYHOFF])
def test_gather_of_translated_genomes_over_the_proteins(monkeypatch, planted, mol):
    """The roles swapped: the packed proteins are the database, the translated genomes' signatures the queries."""
    monkeypatch.delenv("KSPIDER_SKETCH", raising=False)
    root = planted[0]
    g_sigs, p_sigs, G, Pr = _sketched(planted, mol)
    engine.pack(str(p_sigs), 3 * K, str(root / f"proteins{mol}.kspack"), 2)
    db, q = [sorted(Pr[p]) for p in PROTEINS], [sorted(G[g]) for g in GENOMES]
    a = [[G[g][h] for h in sorted(G[g])] for g in GENOMES]
    # plain gather
    want = _gather_tsv(db, q, PROTEINS, GENOMES)
    lines = [ln.split("\t") for ln in want.decode().splitlines()[1:]]
    for g in GENOMES:                               # min_hashes is small enough: each genome reports both of its proteins
        assert {"p" + g[1] + "f", "p" + g[1] + "r"} <= {ln[2] for ln in lines if ln[0] == g}
    for n, database in enumerate((root / f"proteins{mol}.kspack", p_sigs)):
        out = str(root / f"GATHER{mol}_{n}")
        engine.gather(str(database), str(g_sigs), 3 * K, out, 2, min_hashes=MIN_HASHES)
        assert open(out + "_kSpider_gather.tsv", "rb").read() == want
    # weighted by the translated genomes' abundances
    want_w, rows = _weighted_tsv(db, q, a, PROTEINS, GENOMES, MIN_HASHES)
    assert len(rows) == len(lines)
    out = str(root / f"WEIGHTED{mol}")
    engine.gather_abund(str(root / f"proteins{mol}.kspack"), str(g_sigs), 3 * K, out, 2, min_hashes=MIN_HASHES)
    got = open(out + "_kSpider_gather.tsv", "rb").read()
    assert got == want_w
    assert [ln.split(b"\t")[:9] for ln in got.splitlines()] == [ln.split(b"\t") for ln in want.splitlines()]

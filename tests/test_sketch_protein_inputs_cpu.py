"""Pins the restatement of the protein sketch definition (tests/sketch_protein_restate.py) by hand-written cases, and checks that
every input builder of tests/sketch_protein_inputs.py contains what it is named for.  Calls nothing of the product but the
tile constant."""
import pytest

import sketch_protein_inputs as I
import sketch_protein_restate as P
from kspider_amd import engine

T = I.TILE


def test_the_tile_constant():
    assert engine.SKETCH_TILE_BASES == T == 4096 and T % 3 == 1 and (2 * T) % 3 == 2


# ---- the restatement

def test_a_hand_translated_window():
    assert P.translate("ATGGCCTAA") == "MA*"
    assert P.revcomp("ATGGCCTAA") == "TTAGGCCAT" and P.translate("TTAGGCCAT") == "LGH"
    assert P.source_kmers(b"ATGGCCTAA", 3, P.PROTEIN, True) == ["MA*", "LGH"]
    assert P.source_kmers(b"atggcctaa", 3, P.DAYHOFF, True) == ["eb*", "ebd"]
    assert P.source_kmers(b"ATGGCCTAA", 3, P.HP, True) == ["hh*", "hhp"]


def test_all_three_frames_of_twelve_bases():
    s = "ATGGCCTAAGTC"   # frames: ATG GCC TAA | TGG CCT AAG | GGC CTA AGT ; then TCA at 9 is not whole at k = 3
    got = P.source_kmers(s.encode(), 3, P.PROTEIN, True)
    assert got == ["MA*", "LGH", "WPK", "LRP", "GLS", "T*A", "A*V", "DLG"]
    # by hand: window 1 TGGCCTAAG -> W P K, its reverse complement CTTAGGCCA -> L R P; window 2 GGCCTAAGT -> G L S,
    # ACTTAGGCC -> T * A; window 3 GCCTAAGTC -> A * V, GACTTAGGC -> D L G
    assert P.n_windows(s.encode(), 3, True) == 4 and P.n_windows(s.encode(), 4, True) == 1 and P.n_windows(s.encode(), 5, True) == 0


def test_every_codon():
    want = {   # the standard code, written out amino acid by amino acid
        "F": "TTT TTC", "L": "TTA TTG CTT CTC CTA CTG", "S": "TCT TCC TCA TCG AGT AGC", "Y": "TAT TAC", "*": "TAA TAG TGA", "C": "TGT TGC",
        "W": "TGG", "P": "CCT CCC CCA CCG", "H": "CAT CAC", "Q": "CAA CAG", "R": "CGT CGC CGA CGG AGA AGG", "I": "ATT ATC ATA", "M": "ATG",
        "T": "ACT ACC ACA ACG", "N": "AAT AAC", "K": "AAA AAG", "V": "GTT GTC GTA GTG", "A": "GCT GCC GCA GCG", "D": "GAT GAC", "E": "GAA GAG",
        "G": "GGT GGC GGA GGG"}
    table = {codon: aa for aa, codons in want.items() for codon in codons.split()}
    assert len(table) == 64
    for codon, aa in table.items():
        assert P.translate_codon(codon) == aa == P.translate_codon(codon.lower()), codon


def test_every_letters_class():
    dayhoff = dict(A="b", B="X", C="a", D="c", E="c", F="f", G="b", H="d", I="e", J="X", K="d", L="e", M="e", N="c", O="X", P="b", Q="c", R="d", S="b", T="b", U="X", V="e",
                   W="f", X="X", Y="f", Z="X")
    hp = dict(A="h", B="X", C="p", D="p", E="p", F="h", G="h", H="p", I="h", J="X", K="p", L="h", M="h", N="p", O="X", P="h", Q="p", R="p", S="p", T="p", U="X", V="h", W="h",
              X="X", Y="h", Z="X")
    for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ":
        assert P.encode(c, P.PROTEIN) == c == P.encode(c.lower(), P.PROTEIN)
        assert P.encode(c, P.DAYHOFF) == dayhoff[c] == P.encode(c.lower(), P.DAYHOFF)
        assert P.encode(c, P.HP) == hp[c] == P.encode(c.lower(), P.HP)
    for mol in (P.PROTEIN, P.DAYHOFF, P.HP):
        assert P.encode("*", mol) == "*"
    sizes = lambda enc, letters: [sum(enc[c] == l for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ") for l in letters]   # noqa: E731
    assert sizes(dayhoff, "abcdef") == [1, 5, 4, 3, 4, 3] and sizes(hp, "hp") == [10, 10]
    assert [c for c in dayhoff if dayhoff[c] == "X"] == list("BJOUXZ") == [c for c in hp if hp[c] == "X"]


def test_counts_and_breaks_of_the_restatement():
    (run,) = P.counted_sketch(b"MKV-MKV*mkv", [0, 11], 3, P.PROTEIN, False, 2**64 - 1)
    h = dict(zip(["MKV", "KV*", "V*M", "*MK"], P.text_hashes(["MKV", "KV*", "V*M", "*MK"])))
    assert run == {h["MKV"]: 3, h["KV*"]: 1, h["V*M"]: 1, h["*MK"]: 1}
    assert P.counted_sketch(b"MK\nV", [0, 4], 3, P.PROTEIN, False, 2**64 - 1) == [{}]
    assert P.counted_sketch(b"MKVMKV", [0, 3, 6], 3, P.PROTEIN, False, 2**64 - 1) == [{h["MKV"]: 1}, {h["MKV"]: 1}]   # no k-mer over the seam


# ---- the builders

def test_protein_mixed_and_all_byte_values():
    c = I.protein_mixed()
    text = c.seq.decode("latin-1")
    assert all(x in text for x in "*BJOUXZ\n7-\0\xff") and any(x.islower() for x in text) and len(c.offsets) == 4
    c = I.all_byte_values()
    assert sorted(set(c.seq)) == list(range(256))
    for b in range(256):
        at = 70 + 71 * b
        assert c.seq[at] == b and all(chr(x) in P.RESIDUES for x in c.seq[at - 70:at])
    assert P.n_windows(c.seq, 64, False) > 256 * 7


def test_dna_mixed():
    c = I.dna_mixed()
    text = c.seq.decode("latin-1")
    assert all(x in text for x in "NnRY\n\0-") and any(x in text for x in "acgt") and P.n_windows(c.seq, 21, True) > 100


@pytest.mark.parametrize("k", I.TRANSLATED_K)
def test_break_at_every_offset(k):
    c = I.break_at_every_offset(k)
    w = 3 * k
    assert len(c.offsets) == w + 1
    for o in range(w):
        src = c.seq[c.offsets[o]:c.offsets[o + 1]]
        assert src[w + o] == ord("N") and src.count(b"N") == 1
        window = src[w:2 * w]
        assert window[o] == ord("N")                               # the fixed window is broken at its offset o
        assert P.n_windows(src, k, True) == (2 * w + 1) - w        # 2w + 1 positions, the w that cover the N are gone


@pytest.mark.parametrize("window,dna", [(3, True), (30, True), (63, True), (1, False), (33, False), (64, False)])
def test_abutting(window, dna):
    for c, b in zip(I.abutting(window, dna=dna), (T - 1, T, T + 1)):
        assert c.offsets[1] == c.offsets[0] == 0 and c.offsets[2] == b                # empty, then A up to the edge
        assert c.offsets[3] - c.offsets[2] == min(window - 1, 5) < window             # shorter than a window
        assert c.offsets[3] == c.offsets[4] and c.offsets[5] == c.offsets[6] == len(c.seq)
        assert all(chr(x) in (P.BASES if dna else P.RESIDUES) for x in c.seq)          # no break byte anywhere


@pytest.mark.parametrize("k", [2, 10])
def test_alike_on_both_strands(k):
    c = I.alike_on_both_strands(k)
    w = c.seq.decode()
    assert len(w) == 3 * k and P.revcomp(w) == w
    a, b = P.source_kmers(c.seq, k, P.PROTEIN, True)
    assert a == b
    assert list(P.counted_sketch(c.seq, c.offsets, k, P.PROTEIN, True, 2**64 - 1)[0].values()) == [2]


@pytest.mark.parametrize("dna", [True, False])
def test_tile_streams_and_three_tiles(dna):
    cases = I.tile_streams(dna=dna)
    assert [len(c.seq) % 16 for c in cases] == list(range(1, 16)) and all(2 * T < len(c.seq) <= 3 * T for c in cases)
    alphabet = P.BASES if dna else P.RESIDUES
    assert all(chr(x) in alphabet for c in cases for x in c.seq)   # no break: the last window ends exactly at the stream's end
    # the windows over a tile edge start at edge - window + 1 .. edge - 1: over the two edges every codon phase for every window
    for k in I.TRANSLATED_K:
        phases = {p % 3 for edge in (T, 2 * T) for p in range(edge - 3 * k + 1, edge)}
        assert phases == {0, 1, 2}, k
    c = I.three_tiles(dna=dna)
    assert len(c.seq) == 3 * T == 12288 and c.seq[2 * T - 1] == 10 and c.offsets == [0, T // 2, T + 77, 3 * T]
    assert sum(chr(x) not in alphabet for x in c.seq) == 1


def test_poly_a():
    c = I.poly_a()
    assert c.seq == b"A" * (T + 2000)
    kmers = P.source_kmers(c.seq[:100], 10, P.PROTEIN, True)
    assert set(kmers[0::2]) == {"K" * 10} and set(kmers[1::2]) == {"F" * 10}


# ---- the builders of the edge tests (tests/test_sketch_protein_edges_gpu.py)

MANY_WINDOWS = [(1, False), (7, False), (16, False), (33, False), (64, False), (3, True), (21, True), (63, True)]   # the windows the edge tests run


@pytest.mark.parametrize("window,dna", MANY_WINDOWS)
def test_many_sources(window, dna):
    c = I.many_sources(window, dna)
    off, n = c.offsets, len(c.seq)
    assert n == 3 * T + 7 and n % 16 and off[0] == 0 and off[-1] == n and off == sorted(off)
    assert all(chr(x) in (P.BASES if dna else P.RESIDUES) for x in c.seq)            # no break byte: the sources abut
    assert 0.05 < sum(chr(x).islower() for x in c.seq) / n < 0.15
    assert {T - 1, T, T + 1, 2 * T} <= set(off)                                        # the forced ends
    assert {x % 16 for x in off[1:]} == set(range(16))                                 # ends at every offset of a 16-byte piece
    assert len(off) - 1 >= 100
    lengths = [b - a for a, b in zip(off, off[1:])]
    assert lengths[:3] == [0, 0, 0] and lengths[-3:] == [0, 0, 0]                      # empty sources at the start and at the end
    at = off.index(2 * T)
    assert off[at:at + 4] == [2 * T] * 4                                               # and three on a tile edge
    assert sum(x == 0 for x in lengths) >= 9 and (window == 1 or sum(0 < x < window for x in lengths) >= 20)
    assert sum(x >= window for x in lengths) >= 20
    # sources lie on both sides of, and over, each tile edge
    for edge in (T, 2 * T, 3 * T):
        assert any(a < edge < b for a, b in zip(off, off[1:])) or edge in off


def test_strand_thresholds():
    c = I.dna_mixed()
    fw, rv = I.strand_hashes(c, 10, P.PROTEIN)
    m1, m2 = I.strand_thresholds(c, 10, P.PROTEIN)
    assert m1 in fw and m1 not in rv and m2 in rv and m2 not in fw                     # both kinds exist
    everything = sorted(fw | rv)
    for m in (m1, m2):                                                                 # neither empty nor full
        assert len(everything) // 10 < sum(h <= m for h in everything) < len(everything) - len(everything) // 10
    m = I.median_hash(I.protein_mixed(), 17, P.PROTEIN, False)
    hashes = {h for run in P.counted_sketch(*I.protein_mixed()[1:], 17, P.PROTEIN, False, 2**64 - 1) for h in run}
    assert m in hashes and 100 < sum(h <= m for h in hashes) < len(hashes) - 100


def test_clean_records_and_six_frames():
    c = I.dna_mixed()
    records = I.clean_records(c)
    assert len(records) > 5 and all(set(r) <= P.BASES for r in records) and sum(map(len, records)) == sum(chr(x) in P.BASES for x in c.seq)
    assert any(len(r) >= 63 for r in records)
    assert I.six_frames(["ATGGCCTAAGTC"]) == b"MA*V\nWPK\nGLS\nDLGH\nT*A\nLRP"   # by hand: the reverse complement is GACTTAGGCCAT


@pytest.mark.parametrize("translated", [False, True])
def test_low_complexity_beats_the_first_capacity(translated):
    """If a change to the guess in sketch_host stops the retry of test_natural_retry, this says why."""
    c = I.low_complexity(translated)
    max_hash = P.max_hash_of(1000)
    guess = I.first_capacity_guess(len(c.seq), max_hash, translated)
    (run,) = P.counted_sketch(c.seq, c.offsets, 8, P.PROTEIN, translated, max_hash)
    (h,) = P.text_hashes(["T" * 8])
    assert h == 72033104883516 <= max_hash
    assert run == {h: 9550 if translated else 12281} and guess == (8262 if translated else 4111)
    assert sum(run.values()) > guess                                                   # survivors > guess
    assert len(c.seq) == (7 if translated else 3) * T


@pytest.mark.parametrize("dna", [False, True])
def test_long_stream(dna):
    c = I.long_stream(5, dna)
    assert len(c.seq) == 5 * T + 9 and c.offsets[0] == 0 and c.offsets[-1] == len(c.seq)
    newlines = [i for i, x in enumerate(c.seq) if x == 10]
    assert [x - 1 for x in c.offsets[1:-1]] == newlines[:len(c.offsets) - 2] and len(newlines) - (len(c.offsets) - 2) in (0, 1)
    gaps = [b - a for a, b in zip([-1] + newlines, newlines)]
    assert min(gaps) >= 300 and max(gaps) <= 700
    assert all(chr(x) in (P.BASES if dna else P.RESIDUES) for x in c.seq if x != 10)


def test_sweep_cases():
    cases = [d for seed in I.SWEEP_SEEDS for d in I.sweep_cases(seed)]
    assert len(cases) == 48 and cases[:12] == I.sweep_cases(I.SWEEP_SEEDS[0])          # seeded
    assert {d["translated"] for d in cases} == {False, True} and {d["mol"] for d in cases} == {P.PROTEIN, P.DAYHOFF, P.HP}
    assert {d["cap"] for d in cases} == {None, "1", "2"} and {d["seed"] for d in cases} == {42, 7} and {d["density"] for d in cases} == {0.0, 1 / 400, 1 / 30}
    assert {0, 2**64 - 1, P.max_hash_of(25)} < {d["max_hash"] for d in cases}          # and hashes that occur
    for d in cases:
        c = d["case"]
        assert 1 <= len(c.seq) <= 2 * T + 64 and 1 <= len(c.offsets) - 1 <= 40 and c.offsets == sorted(c.offsets) and c.offsets[0] == 0 and c.offsets[-1] == len(c.seq)
        assert d["k"] in (I.TRANSLATED_K if d["translated"] else I.RESIDUE_K)
    assert any(a == b for d in cases for a, b in zip(d["case"].offsets, d["case"].offsets[1:]))   # empty sources
    assert any(len(d["case"].seq) > T for d in cases) and any(len(d["case"].seq) < T for d in cases)

"""Seeded inputs of the protein-sketch tests (CPU and GPU).  Every builder returns Case(name, seq, offsets) — a byte stream and
the bounds of its sources — or a list of them, and says what it is named for; tests/test_sketch_protein_inputs_cpu.py checks
that each really contains that."""
import random

from sketch_inputs import TILE, Case, bases
import sketch_protein_restate as P

AMINO = "ACDEFGHIKLMNPQRSTVWY"
RESIDUE_K = [1, 7, 8, 9, 15, 16, 17, 32, 33, 64]   # Murmur's word, block and tail boundaries
TRANSLATED_K = [1, 2, 7, 10, 11, 21]               # 3k = 33 crosses the packed word, 63 is the limit


def residues(rng, n, lower=0.0):
    """n random residues of the 20 amino acids; a share `lower` of them in lower case."""
    return "".join(c.lower() if lower and rng.random() < lower else c for c in (rng.choice(AMINO) for _ in range(n)))


def protein_mixed(n=1500, seed=41):
    """Named for its mixture: amino acids in both cases, '*', the letters B J O U X Z that the reduced alphabets turn into X, and
    break bytes (newline, digit, '-', a zero byte, 0xFF); three sources of uneven length."""
    rng = random.Random(seed)
    s = list(residues(rng, n, lower=0.3))
    specials = "*BJOUXZbz*\n7-\0\xff*"
    for i in range(max(n // 60, len(specials))):
        s[rng.randrange(n)] = specials[i % len(specials)]
    cuts = sorted(rng.randrange(1, n) for _ in range(2))
    return Case("protein_mixed", "".join(s).encode("latin-1"), [0] + cuts + [n])


def all_byte_values(seed=42, run=70):
    """Named for the 256 byte values: each one once, behind a run of 70 amino acids, so that for every k <= 64 each value is met
    as the last, a middle and the first byte of windows (or breaks them)."""
    rng = random.Random(seed)
    out = bytearray()
    for b in range(256):
        out += residues(rng, run).encode() + bytes([b])
    out += residues(rng, run).encode()
    return Case("all_byte_values", bytes(out), [0, len(out)])


def dna_mixed(n=1500, seed=43):
    """Named for its mixture: bases in both cases, N and other IUPAC codes, newlines, a zero byte; three sources."""
    rng = random.Random(seed)
    s = list(bases(rng, n, lower=0.3))
    specials = "NnRY\n\0-"
    for i in range(max(n // 250, len(specials))):
        s[rng.randrange(n)] = specials[i % len(specials)]
    cuts = sorted(rng.randrange(1, n) for _ in range(2))
    return Case("dna_mixed", "".join(s).encode("latin-1"), [0] + cuts + [n])


def break_at_every_offset(k, seed=44):
    """Named for the non-ACGT byte at every offset 0 .. 3k - 1 of one fixed window: source o is the same 9k bases with an N at
    3k + o, so the window at 3k is broken at its offset o, and the windows before and behind the N are whole."""
    rng = random.Random(seed * 1000 + k)
    w = 3 * k
    whole = bases(rng, 3 * w)
    parts = [whole[:w + o] + "N" + whole[w + o + 1:] for o in range(w)]
    return Case(f"break_at_every_offset_k{k}", "".join(parts).encode(), [3 * w * i for i in range(w + 1)])


def abutting(window, seed=45, tile=TILE, dna=True):
    """Named for sources that abut without a break byte: [empty, A, short, empty, B, empty] with the end of A exactly on, one
    before and one behind a tile edge; `short` has fewer bytes than a window (window > 1).  dna: bases, else amino acids."""
    rng = random.Random(seed * 1000 + window)
    whole = bases(rng, tile + 300) if dna else residues(rng, tile + 300)
    out = []
    for b in (tile - 1, tile, tile + 1):
        short = min(window - 1, 5)
        off = [0, 0, b, b + short, b + short, b + short + 200, b + short + 200]
        out.append(Case(f"abutting_at{b}", whole[:off[-1]].encode(), off))
    return out


def alike_on_both_strands(k, seed=46):
    """Named for a window that is its own reverse complement (k even, so 3k is): both strands translate to the same k-mer, whose
    count is therefore 2.  The window is the whole source."""
    assert k % 2 == 0
    rng = random.Random(seed * 1000 + k)
    half = bases(rng, 3 * k // 2)
    w = half + P.revcomp(half)
    return Case(f"alike_on_both_strands_k{k}", w.encode(), [0, len(w)])


def tile_streams(seed=47, tile=TILE, dna=True):
    """Named for the stream's end: one source without a break of 2 tile + r bytes, r = 1 .. 15, so the stream ends r bytes into a
    16-byte piece; the last window ends exactly at the stream's end, and the positions behind it would need bytes beyond it.
    Windows lie over both tile edges (4 096 and 8 192, neither a multiple of 3) in every codon phase the window length allows."""
    rng = random.Random(seed)
    whole = bases(rng, 2 * tile + 15, lower=0.1) if dna else residues(rng, 2 * tile + 15, lower=0.1)
    return [Case(f"stream_ends_{r}_into_a_piece", whole[:2 * tile + r].encode(), [0, 2 * tile + r]) for r in range(1, 16)]


def three_tiles(seed=48, tile=TILE, dna=True):
    """Named for its length, 3 tile bytes exactly (12 288): three sources that abut in the middle of tiles, one break byte on each
    tile edge's left neighbour in the second half, so windows cross the first edge and are broken at the second."""
    rng = random.Random(seed)
    s = list(bases(rng, 3 * tile, lower=0.1) if dna else residues(rng, 3 * tile, lower=0.1))
    s[2 * tile - 1] = "\n"
    return Case("three_tiles", "".join(s).encode(), [0, tile // 2, tile + 77, 3 * tile])


def poly_a(tile=TILE):
    """Named for one hash repeated some thousand times over a tile edge: tile + 2 000 times A.  Translated, every window is
    KKK... on the forward strand and FFF... on the reverse strand."""
    n = tile + 2000
    return Case("poly_a", b"A" * n, [0, n])

"""Seeded inputs of the protein-sketch tests (CPU and GPU).  Every builder returns Case(name, seq, offsets) — a byte stream and
the bounds of its sources — or a list of them, and says what it is named for; tests/test_sketch_protein_inputs_cpu.py checks
that each really contains that.  Beside the builders: thresholds, records and frames derived from a case by the restatement, the
first-capacity formula, and the parameter sets of the seeded sweep."""
import random

import numpy as np

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


def many_sources(window, dna, seed=49, tile=TILE):
    """Named for the shape of a proteome: one stream of 3 tile + 7 bytes (ending 7 bytes into a 16-byte piece) without a break
    byte, a tenth of it in lower case, cut into sources that abut.  The lengths are drawn from 0, 1, window - 1, window,
    window + 1, 2 window, 2 window + 3 and 5 window (window 1: without the lengths that are not positive), so sources are empty or
    shorter than a window by the hundred.  Source ends are forced at tile - 1, tile, tile + 1 and 2 tile, and four empty sources
    each sit at the start, on the tile edge 2 tile and at the end."""
    rng = random.Random(seed * 1000 + window + (500 if dna else 0))
    n = 3 * tile + 7
    text = bases(rng, n, lower=0.1) if dna else residues(rng, n, lower=0.1)
    lengths = [0, 1, window - 1, window, window + 1, 2 * window, 2 * window + 3, 5 * window]
    if window == 1:
        lengths = [x for x in lengths if x > 0]
    cuts, at = [], 0
    while True:
        at += rng.choice(lengths)
        if at >= n:
            break
        cuts.append(at)
    forced = [tile - 1, tile, tile + 1, 2 * tile]
    offsets = sorted([0] * 5 + cuts + forced + [2 * tile] * 4 + [n] * 5)
    return Case(f"many_sources_w{window}_{'dna' if dna else 'protein'}", text.encode(), offsets)


def strand_hashes(case, k, mol, seed=42):
    """(the hashes of the k-mers that occur as a forward translation inside a source of the case, those that occur as a reverse
    translation), by the restatement."""
    fw, rv = set(), set()
    for s in range(len(case.offsets) - 1):
        kmers = P.source_kmers(case.seq[case.offsets[s]:case.offsets[s + 1]], k, mol, True)
        fw |= set(P.text_hashes(kmers[0::2], seed)) if kmers else set()
        rv |= set(P.text_hashes(kmers[1::2], seed)) if kmers else set()
    return fw, rv


def strand_thresholds(case, k, mol):
    """Named for a threshold that only one strand reaches: (m1, m2), m1 the median of the hashes that occur in the case only as a
    forward translation, m2 the median of those that occur only as a reverse translation.  At max_hash = m1 some position's
    forward hash is exactly at the threshold and no reverse hash is; at m2 the reverse."""
    fw, rv = strand_hashes(case, k, mol)
    only_f, only_r = sorted(fw - rv), sorted(rv - fw)
    return only_f[len(only_f) // 2], only_r[len(only_r) // 2]


def median_hash(case, k, mol, translated):
    """The median of the distinct hashes of a case, by the restatement: a threshold that keeps the sketch neither empty nor full."""
    hashes = sorted({h for run in P.counted_sketch(case.seq, case.offsets, k, mol, translated, 2**64 - 1) for h in run})
    return hashes[len(hashes) // 2]


def clean_records(case):
    """Named for records free of breaks: the stream of a DNA case cut at every byte outside ACGTacgt, the pieces as a list of str."""
    out, cur = [], []
    for c in case.seq.decode("latin-1"):
        if c in P.BASES:
            cur.append(c)
        elif cur:
            out.append("".join(cur))
            cur = []
    return out + (["".join(cur)] if cur else [])


def six_frames(records):
    """The six frame translations of every record, joined by newlines: protein input as one source."""
    frames = [P.translate(s[f:]) for r in records for s in (r, P.revcomp(r)) for f in range(3)]
    return "\n".join(frames).encode()


def first_capacity_guess(n_bytes, max_hash, translated):
    """The first capacity of ksp_sketch_host_mol (csrc/sketcher.hip, sketch_host), recomputed: per = 2 for translated input, else 1;
    min(per * n_bytes, per * (floor(n_bytes * (max_hash + 1) / 2^64 * 1.25) + 4096))."""
    per = 2 if translated else 1
    share = (float(max_hash) + 1.0) / 18446744073709551616.0
    return min(per * n_bytes, per * (int(float(n_bytes) * share * 1.25) + 4096))


def low_complexity(translated, tile=TILE):
    """Named for beating the first-capacity guess at scaled 1000 and k = 8 by low complexity: T times 3 tile as protein input (one
    k-mer, TTTTTTTT, at 12 281 positions; the guess is 4 111), or ACC repeated to 7 tile bases as translated input (frame 0 of the
    forward strand is TTTTTTTT at 9 550 positions, the five other k-mers' hashes lie above the threshold; the guess is 8 262)."""
    if not translated:
        return Case("poly_t", b"T" * (3 * tile), [0, 3 * tile])
    n = 7 * tile
    return Case("acc_repeat", ("ACC" * (n // 3 + 1))[:n].encode(), [0, n])


def long_stream(n_tiles, dna, seed=50, tile=TILE):
    """Named for more tiles than the default grid has workgroups: n_tiles tile + 9 random bytes (bases or amino acids, upper case)
    with a newline every 300 to 700 bytes; every newline ends a source."""
    rng = np.random.default_rng(seed + (1 if dna else 0))
    n = n_tiles * tile + 9
    alphabet = np.frombuffer(("ACGT" if dna else AMINO).encode(), dtype=np.uint8)
    seq = alphabet[rng.integers(0, alphabet.size, size=n)]
    gaps = rng.integers(300, 701, size=n // 300 + 1)
    at = np.cumsum(gaps) - 1                  # the newlines' positions: the first after 299 .. 699 bytes
    at = at[at < n]
    seq[at] = 10
    offsets = [0] + (at + 1).tolist()
    if offsets[-1] != n:
        offsets.append(n)
    return Case(f"long_stream_{n_tiles}_tiles", seq.tobytes(), offsets)


SWEEP_SEEDS = [101, 102, 103, 104]


def sweep_cases(seed, n=12, tile=TILE):
    """Named for nothing in particular: n seeded random cases as dicts (case, k, mol, translated, max_hash, seed, cap, density).
    Each draws a length in [1, 2 tile + 64], translated or not, a molecule type, k from the module's lists, a density of break
    bytes from 0, 1/400 and 1/30, 1 to 40 sources with random cuts (empty ones allowed), max_hash from all ones, scaled 25, a hash
    that occurs in the case (all ones where none does) and 0, a hash seed from 42 and 7, a workgroup cap from unset, "1", "2"."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        length = rng.randint(1, 2 * tile + 64)
        translated = rng.random() < 0.5
        mol = rng.choice([P.PROTEIN, P.DAYHOFF, P.HP])
        k = rng.choice(TRANSLATED_K if translated else RESIDUE_K)
        density = rng.choice([0.0, 1 / 400, 1 / 30])
        s = list(bases(rng, length, lower=0.2) if translated else residues(rng, length, lower=0.2))
        for j in range(length):
            if density and rng.random() < density:
                s[j] = rng.choice("\nN-\0" if translated else "\n7-\0")
        cuts = sorted(rng.randint(0, length) for _ in range(rng.randint(1, 40) - 1))
        case = Case(f"sweep_{seed}_{i}", "".join(s).encode("latin-1"), [0] + cuts + [length])
        hash_seed = rng.choice([42, 7])
        which = rng.choice(["full", "few", "occurring", "zero"])
        pick = rng.random()
        if which == "occurring":
            hashes = sorted({h for run in P.counted_sketch(case.seq, case.offsets, k, mol, translated, 2**64 - 1, hash_seed) for h in run})
            max_hash = hashes[int(pick * len(hashes))] if hashes else 2**64 - 1
        else:
            max_hash = {"full": 2**64 - 1, "few": P.max_hash_of(25), "zero": 0}[which]
        out.append(dict(case=case, k=k, mol=mol, translated=translated, max_hash=max_hash, seed=hash_seed, cap=rng.choice([None, "1", "2"]), density=density))
    return out

"""Seeded inputs of the sketch tests (CPU and GPU).  Every generator returns Case(name, seq, offsets) — a byte stream and the
bounds of its sources — or a list of them; tests/test_sketch_inputs_cpu.py checks that each really contains what it claims."""
import random
from collections import namedtuple

import sketch_restate as R

Case = namedtuple("Case", "name seq offsets")

TILE = 4096   # KSP_SKETCH_TILE_BASES (checked against engine.SKETCH_TILE_BASES by the input tests)


def bases(rng, n, lower=0.0):
    """n random bases; a share `lower` of them in lower case."""
    out = []
    for _ in range(n):
        c = rng.choice("ACGT")
        out.append(c.lower() if lower and rng.random() < lower else c)
    return "".join(out)


def mixed(n=3000, seed=11, n_sources=3):
    """About n bytes: bases in both cases, N and other IUPAC codes, a zero byte, newlines; n_sources sources of uneven length."""
    rng = random.Random(seed)
    s = list(bases(rng, n, lower=0.3))
    specials = "NnRYKM\n\0-"
    for i in range(max(n // 150, len(specials))):
        s[rng.randrange(n)] = specials[i % len(specials)]
    cuts = sorted(rng.randrange(1, n) for _ in range(n_sources - 1))
    return Case("mixed", "".join(s).encode("latin-1"), [0] + cuts + [n])


def tile_lengths(k, tile=TILE):
    return [tile - 1, tile, tile + 1, tile + k - 1, 2 * tile + 1]


def tile_edges(k, seed=12, tile=TILE):
    """One source of tile - 1, tile, tile + 1, tile + k - 1 and 2 tile + 1 bases, each without a break and with one break byte at
    tile - 1, at tile and at tile + k - 2 (where the source is that long).  All are cut from one random sequence, so that a
    reference hashes most k-mers once."""
    rng = random.Random(seed * 1000 + k)
    whole = bases(rng, 2 * tile + 1, lower=0.1)
    out = []
    for n in tile_lengths(k, tile):
        for at in (None, tile - 1, tile, tile + k - 2):
            if at is not None and at >= n:
                continue
            s = whole[:n] if at is None else whole[:at] + "N" + whole[at + 1:n]
            out.append(Case(f"edge_len{n}_break{at}", s.encode(), [0, n]))
    return out


def boundaries(k, seed=13, tile=TILE):
    """Sources that abut without a break byte: [empty, A, short, empty, B, empty] with the end of A exactly on, one before and
    one behind a tile edge; `short` has fewer than k bases (k > 1)."""
    rng = random.Random(seed * 1000 + k)
    whole = bases(rng, tile + 300)
    out = []
    for b in (tile - 1, tile, tile + 1):
        short = min(k - 1, 5)
        off = [0, 0, b, b + short, b + short, b + short + 200, b + short + 200]
        out.append(Case(f"boundary_at{b}", whole[:off[-1]].encode(), off))
    return out


def junction(k, seed=14):
    """Two sources of 150 bases that abut: the k - 1 windows over the junction spell k-mers that neither source contains."""
    rng = random.Random(seed * 1000 + k)
    return Case("junction", bases(rng, 300).encode(), [0, 150, 300])


def short_reads(n_reads=2000, seed=15):
    """n_reads reads of 40 to 150 bases, each followed by a newline: (one source, one source per read)."""
    rng = random.Random(seed)
    reads = [bases(rng, rng.randint(40, 150)) + "\n" for _ in range(n_reads)]
    seq = "".join(reads).encode()
    off = [0]
    for r in reads:
        off.append(off[-1] + len(r))
    return Case("reads_one_source", seq, [0, len(seq)]), Case("reads_as_sources", seq, off)


def duplicates(k, seed=16):
    """(a sequence twice in one source, separated by a break; one sequence in two sources; a sequence and its reverse complement
    as two sources)."""
    rng = random.Random(seed * 1000 + k)
    a = bases(rng, 400)
    twice = Case("twice_in_one", (a + "N" + a).encode(), [0, 2 * len(a) + 1])
    shared = Case("shared_by_two", (a + a).encode(), [0, len(a), 2 * len(a)])
    mirror = Case("with_revcomp", (a + R.revcomp(a)).encode(), [0, len(a), 2 * len(a)])
    return twice, shared, mirror


def palindrome(k, seed=17):
    """For even k: a k-mer that is its own reverse complement, between random flanks."""
    assert k % 2 == 0
    rng = random.Random(seed * 1000 + k)
    half = bases(rng, k // 2)
    pal = half + R.revcomp(half)
    s = bases(rng, 40) + pal + bases(rng, 40)
    return Case("palindrome", s.encode(), [0, len(s)]), pal


def ordered_pair(k, seed=18):
    """(a k-mer that is smaller than its reverse complement, one that is larger), each alone in a source."""
    rng = random.Random(seed * 1000 + k)
    while True:
        x = bases(rng, k)
        if x != R.revcomp(x):
            break
    small, large = sorted((x, R.revcomp(x)))
    return Case("smaller_and_larger", (small + large).encode(), [0, k, 2 * k]), small, large


def all_cases(k):
    """Every case a ksize takes part in (the CPU comparison runs them all)."""
    out = [mixed()] + list(duplicates(k)) + [junction(k), ordered_pair(k)[0]]
    if k % 2 == 0:
        out.append(palindrome(k)[0])
    return out

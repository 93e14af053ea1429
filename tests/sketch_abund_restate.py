"""Counted sketches, restated (include/kspider_amd.h, "Counted sketches"): the abundance of a kept hash in a source is the number
of its k-mers — tests/sketch_restate.py's enumeration, which this module only counts with collections.Counter — that have that
hash, forward and reverse-complement occurrences together, clamped at 2^32 - 1.  Shares no code with the library.  Also the
inputs of the counted tests: Case(name, seq, offsets) as tests/sketch_inputs.py makes them."""
import random
from collections import Counter

import numpy as np

import sketch_inputs as I
import sketch_restate as R

CLAMP = 2**32 - 1


def sketch(seq: bytes, src_offsets, ksize: int, max_hash: int, seed: int = 42) -> list:
    """Per source the ascending list of (hash, abundance)."""
    out = []
    for s in range(len(src_offsets) - 1):
        text = bytes(seq[int(src_offsets[s]):int(src_offsets[s + 1])])
        count = Counter(h for h in R.source_hashes(text, ksize, seed) if h <= max_hash)
        out.append(sorted((h, min(n, CLAMP)) for h, n in count.items()))
    return out


def flat(sketches) -> tuple:
    """(keys, abund, offsets) as the library returns them."""
    keys = np.array([h for run in sketches for h, _ in run], dtype=np.uint64)
    abund = np.array([n for run in sketches for _, n in run], dtype=np.uint32)
    off = np.zeros(len(sketches) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(run) for run in sketches])
    return keys, abund, off


def homopolymer(k, length=300):
    """One source of `length` A: one hash, length - k + 1 times"""
    return I.Case("homopolymer", b"A" * length, [0, length])


def mirror(k, seed=41):
    """One source: a k-mer, a break, its reverse complement, a break, the k-mer again: one hash three times (a palindrome aside)"""
    rng = random.Random(seed)
    kmer = I.bases(rng, k)
    seq = (kmer + "N" + R.revcomp(kmer) + "\n" + kmer.lower()).encode()
    return I.Case("mirror", seq, [0, len(seq)])


def abutting(k, seed=42):
    """Two sources without a break byte between them that share a k-mer: the first holds it twice, the second once; no window
    over the boundary counts for either"""
    rng = random.Random(seed)
    kmer = I.bases(rng, k)
    a = kmer + "N" + I.bases(rng, 50) + "N" + kmer
    b = kmer + I.bases(rng, 40)
    return I.Case("abutting", (a + b).encode(), [0, len(a), len(a) + len(b)])


def repeat_over_tile_edge(k, period=7, seed=43, tile=I.TILE):
    """A tandem repeat of `period` bases from tile - 200 to tile + 200 inside random bases (2 tiles and a bit): the same few
    hashes on both sides of the tile boundary, so a run of equal survivors comes from two tiles"""
    rng = random.Random(seed)
    unit = I.bases(rng, period)
    seq = I.bases(rng, tile - 200) + (unit * (400 // period + 1))[:400] + I.bases(rng, tile + 300)
    return I.Case("repeat_over_tile_edge", seq.encode(), [0, len(seq)])


def reads(depth_of=((0, 1), (1, 6), (2, 25)), length=600, read_len=80, seed=44):
    """Three genomes of `length` bases sampled as reads at depths 1, 6 and 25 into one source, and the same again split into
    three sources of uneven size: counts well above 1, many of them different"""
    rng = random.Random(seed)
    genomes = [I.bases(rng, length) for _ in depth_of]
    out = []
    for g, depth in depth_of:
        for _ in range(depth * length // read_len):
            at = rng.randrange(length - read_len)
            r = genomes[g][at:at + read_len]
            out.append(R.revcomp(r) if rng.random() < 0.5 else r)
    rng.shuffle(out)
    seq = "".join(r + "\n" for r in out).encode()
    cuts = [0, len(seq) // 5, len(seq) // 2, len(seq)]
    return I.Case("reads_one", seq, [0, len(seq)]), I.Case("reads_three", seq, cuts)

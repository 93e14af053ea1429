"""An independent restatement of the protein, dayhoff and hp sketch definition (include/kspider_amd.h, "protein, dayhoff and hp
sketches"), for the tests: translation from the 64-letter string of the standard genetic code, the encodings as dicts, windows
by slicing Python strings, counts by a Counter.  Murmur and max_hash come from tests/sketch_restate.py (pinned there by
published anchors).  Nothing here calls the product; tests/test_sketch_protein_inputs_cpu.py pins it by hand-written cases."""
from collections import Counter

import numpy as np

from sketch_restate import max_hash_of, murmur3_rows  # noqa: F401  (max_hash_of: for the tests that import this module)

PROTEIN, DAYHOFF, HP = 1, 2, 3
NAMES = {PROTEIN: "protein", DAYHOFF: "dayhoff", HP: "hp"}

#: indexed by 16 b1 + 4 b2 + b3 with T, C, A, G = 0 .. 3
GENETIC_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_TCAG = {"T": 0, "C": 1, "A": 2, "G": 3}
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
_LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"

_DAYHOFF_CLASSES = {"a": "C", "b": "AGPST", "c": "DENQ", "d": "HKR", "e": "ILMV", "f": "FWY"}
_HP_CLASSES = {"h": "AFGILMPVWY", "p": "NCSTDERHKQ"}


def _encoding(classes):
    out = {c: "X" for c in _LETTERS}
    for letter, members in classes.items():
        for c in members:
            out[c] = letter
    out["*"] = "*"
    return out


ENCODING = {PROTEIN: {**{c: c for c in _LETTERS}, "*": "*"}, DAYHOFF: _encoding(_DAYHOFF_CLASSES), HP: _encoding(_HP_CLASSES)}
RESIDUES = set(_LETTERS) | set(_LETTERS.lower()) | {"*"}
BASES = set("ACGTacgt")


def encode(residues: str, mol: int) -> str:
    """The letters that are hashed for a string of residues."""
    return "".join(ENCODING[mol][c] for c in residues.upper())


def translate_codon(codon: str) -> str:
    b1, b2, b3 = (_TCAG[c] for c in codon.upper())
    return GENETIC_CODE[16 * b1 + 4 * b2 + b3]


def translate(dna: str) -> str:
    """The residues of the codons at offsets 0, 3, ... of a string of bases (a trailing one or two bases are dropped)."""
    return "".join(translate_codon(dna[i:i + 3]) for i in range(0, len(dna) - 2, 3))


def revcomp(dna: str) -> str:
    return dna.upper().translate(_COMPLEMENT)[::-1]


_hash_cache = {}


def text_hashes(texts, seed: int = 42) -> list:
    """The hash of every string of encoded letters of a list (all of one length)."""
    todo = sorted({t for t in texts if (t, seed) not in _hash_cache})
    if todo:
        rows = np.frombuffer("".join(todo).encode(), dtype=np.uint8).reshape(len(todo), len(todo[0]))
        h1, _ = murmur3_rows(rows, seed)
        for t, h in zip(todo, h1):
            _hash_cache[(t, seed)] = int(h)
    return [_hash_cache[(t, seed)] for t in texts]


def _windows(text: bytes, length: int, alphabet) -> list:
    """Every (position, slice) of `length` consecutive bytes of `alphabet` in one source."""
    s = text.decode("latin-1")
    return [(i, s[i:i + length]) for i in range(len(s) - length + 1) if all(c in alphabet for c in s[i:i + length])]


def source_kmers(text: bytes, k: int, mol: int, translated: bool) -> list:
    """The encoded k-mers of one source, in order of position, repeats included: one per window of k residues, or for translated
    input two per window of 3k bases (the forward strand's, then the reverse strand's)."""
    if not translated:
        return [encode(w, mol) for _, w in _windows(text, k, RESIDUES)]
    out = []
    for _, w in _windows(text, 3 * k, BASES):
        out.append(encode(translate(w), mol))
        out.append(encode(translate(revcomp(w)), mol))
    return out


def n_windows(text: bytes, k: int, translated: bool) -> int:
    """The windows of one source (of 3k bases, or of k residues), counted by the run of good bytes that ends at each position."""
    length, alphabet = (3 * k, BASES) if translated else (k, RESIDUES)
    run = n = 0
    for c in text.decode("latin-1"):
        run = run + 1 if c in alphabet else 0
        n += run >= length
    return n


def counted_sketch(seq: bytes, src_offsets, k: int, mol: int, translated: bool, max_hash: int, seed: int = 42) -> list:
    """One {hash: abundance} per source, abundances clamped at 2^32 - 1."""
    out = []
    for s in range(len(src_offsets) - 1):
        text = bytes(seq[int(src_offsets[s]):int(src_offsets[s + 1])])
        kmers = source_kmers(text, k, mol, translated)
        counts = Counter(h for h in text_hashes(kmers, seed) if h <= max_hash) if kmers else Counter()
        out.append({h: min(c, 2**32 - 1) for h, c in counts.items()})
    return out


def flat(counted) -> tuple:
    """(keys, abund, offsets) as the library returns them."""
    keys = np.array([h for run in counted for h in sorted(run)], dtype=np.uint64)
    abund = np.array([run[h] for run in counted for h in sorted(run)], dtype=np.uint32)
    off = np.zeros(len(counted) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(run) for run in counted])
    return keys, abund, off

"""An independent restatement of the sketch definition (include/kspider_amd.h, "sketching"), for the tests: MurmurHash3_x64_128 in
numpy uint64 arithmetic, the canonical form by comparing Python strings, selection and sets in plain Python.  Nothing here
shares code with the library.  Checked against two published anchors by tests/test_sketch_cpu.py: SMHasher's verification value
0x6384BA69 and ("foo", seed 0) -> (-2129773440516405919, 9128664383759220103)."""
import numpy as np

_U = np.uint64
_C1, _C2 = _U(0x87C37B91114253D5), _U(0x4CF5AD432745937F)
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
BASES = set("ACGTacgt")


def _rotl(x, r):
    return (x << _U(r)) | (x >> _U(64 - r))


def _fmix(k):
    k ^= k >> _U(33)
    k *= _U(0xFF51AFD7ED558CCD)
    k ^= k >> _U(33)
    k *= _U(0xC4CEB9FE1A85EC53)
    k ^= k >> _U(33)
    return k


def _le(rows, a, b):
    """bytes a .. b - 1 of every row as a little-endian word"""
    k = np.zeros(rows.shape[0], dtype=_U)
    for i in range(b - 1, a - 1, -1):   # (the order of the original's switch: the highest byte first)
        k ^= rows[:, i].astype(_U) << _U(8 * (i - a))
    return k


def murmur3_rows(rows: np.ndarray, seed: int = 0) -> tuple:
    """MurmurHash3_x64_128 of every row of an (n, length) uint8 array: (h1[n], h2[n])."""
    rows = np.asarray(rows, dtype=np.uint8)
    count, n = rows.shape
    with np.errstate(over="ignore"):
        h1 = np.full(count, seed, dtype=_U)
        h2 = np.full(count, seed, dtype=_U)
        blocks = n // 16
        for b in range(blocks):
            k1 = _le(rows, 16 * b, 16 * b + 8)
            k2 = _le(rows, 16 * b + 8, 16 * b + 16)
            k1 *= _C1; k1 = _rotl(k1, 31); k1 *= _C2; h1 ^= k1
            h1 = _rotl(h1, 27); h1 += h2; h1 = h1 * _U(5) + _U(0x52DCE729)
            k2 *= _C2; k2 = _rotl(k2, 33); k2 *= _C1; h2 ^= k2
            h2 = _rotl(h2, 31); h2 += h1; h2 = h2 * _U(5) + _U(0x38495AB5)
        t0, left = 16 * blocks, n - 16 * blocks
        if left > 8:    # cases 15 .. 9 of the original's switch
            k2 = _le(rows, t0 + 8, n)
            k2 *= _C2; k2 = _rotl(k2, 33); k2 *= _C1; h2 ^= k2
        if left > 0:    # cases 8 .. 1
            k1 = _le(rows, t0, t0 + min(left, 8))
            k1 *= _C1; k1 = _rotl(k1, 31); k1 *= _C2; h1 ^= k1
        h1 ^= _U(n); h2 ^= _U(n)
        h1 += h2; h2 += h1
        h1 = _fmix(h1); h2 = _fmix(h2)
        h1 += h2; h2 += h1
        return h1, h2


def murmur3_x64_128(data: bytes, seed: int = 0) -> tuple:
    """(h1, h2) as unsigned Python ints."""
    h1, h2 = murmur3_rows(np.frombuffer(bytes(data), dtype=np.uint8).reshape(1, len(data)), seed)
    return int(h1[0]), int(h2[0])


def smhasher_verification() -> int:
    """SMHasher's VerificationTest for a 128-bit hash: keys {0, 1, ..., i - 1} with seed 256 - i, i = 0 .. 255; the 256 results
    hashed with seed 0; the first four bytes, little-endian."""
    out = b""
    for i in range(256):
        h1, h2 = murmur3_x64_128(bytes(range(i)), 256 - i)
        out += h1.to_bytes(8, "little") + h2.to_bytes(8, "little")
    h1, _ = murmur3_x64_128(out, 0)
    return h1 & 0xFFFFFFFF


def max_hash_of(scaled: int) -> int:
    if scaled < 1:
        raise ValueError("scaled is 1 or more")
    return 2**64 - 1 if scaled == 1 else int(18446744073709551616.0 / float(scaled))


def revcomp(text: str) -> str:
    return text.upper().translate(_COMPLEMENT)[::-1]


def canonical(kmer: str) -> str:
    up = kmer.upper()
    rc = revcomp(up)
    return up if up <= rc else rc   # a comparison of strings


_hash_cache = {}


def kmer_hashes(kmers, seed: int = 42) -> list:
    """The hash of every k-mer of a list (all of one length)."""
    canon = [canonical(k) for k in kmers]
    todo = sorted({c for c in canon if (c, seed) not in _hash_cache})
    if todo:
        rows = np.frombuffer("".join(todo).encode(), dtype=np.uint8).reshape(len(todo), len(todo[0]))
        h1, _ = murmur3_rows(rows, seed)
        for c, h in zip(todo, h1):
            _hash_cache[(c, seed)] = int(h)
    return [_hash_cache[(c, seed)] for c in canon]


def kmer_hash(kmer: str, seed: int = 42) -> int:
    return kmer_hashes([kmer], seed)[0]


def source_kmers(text: bytes, ksize: int) -> list:
    """Every k-mer of one source as (position, text), in order of position."""
    s = text.decode("latin-1")
    out = []
    run = 0   # bases since the last break
    for i, c in enumerate(s):
        run = run + 1 if c in BASES else 0
        if run >= ksize:
            out.append((i - ksize + 1, s[i - ksize + 1:i + 1]))
    return out


def source_hashes(text: bytes, ksize: int, seed: int = 42) -> list:
    """The hash of every k-mer of one source, in order of position (with repeats)."""
    return kmer_hashes([k for _, k in source_kmers(text, ksize)], seed)


def sketch(seq: bytes, src_offsets, ksize: int, max_hash: int, seed: int = 42) -> list:
    """One ascending list of distinct kept hashes per source."""
    out = []
    for s in range(len(src_offsets) - 1):
        text = bytes(seq[int(src_offsets[s]):int(src_offsets[s + 1])])
        out.append(sorted({h for h in source_hashes(text, ksize, seed) if h <= max_hash}))
    return out


def flat(sketches) -> tuple:
    """(keys, offsets) as the library returns them."""
    keys = np.array([h for run in sketches for h in run], dtype=np.uint64)
    off = np.zeros(len(sketches) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(run) for run in sketches])
    return keys, off

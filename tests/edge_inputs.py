"""Restatements of the engine's bucket functions (CPU, integers only) and inputs built to sit on its size thresholds.

The hand-written partition (partition_kernels.hip.h: part_prep / part_bucket) puts key k into bucket umulhi(k, mult),
mult = floor(nb * 2^64 / (maxkey + 1)); every key is its own bucket when maxkey <= nb, and mult = nb when maxkey is
2^64 - 1.  The library partition (engine.hip, grouping by hash bucket) takes the pb bits just below `topbit`.  The
segment partition gives every bucket a fixed range of seg_cap places (engine.hip, the segment partition's setup).
"""
import numpy as np

M64 = (1 << 64) - 1
ALL_ONES = M64
HB_CAP = 3072
HB_MEAN = 800


# ---- the hand-written partition ------------------------------------------------------------------------------------
def hand_nbuckets(n: int, mean: int) -> int:
    """Buckets for n entries at KSP_DEBUG_BUCKET_MEAN=mean (the engine takes at least 8)."""
    mean = max(8, int(mean))
    return max(1, (int(n) + mean - 1) // mean)


def hand_mult(maxkey: int, nb: int):
    """(mult, ident) as part_prep computes them."""
    maxkey, nb = int(maxkey), int(nb)
    if maxkey <= nb:
        return 0, 1
    if maxkey == M64:
        return nb, 0
    return (nb << 64) // (maxkey + 1), 0


def _umulhi(keys: np.ndarray, mult: int) -> np.ndarray:
    """High 64 bits of keys x mult, exactly (32-bit halves in uint64 arithmetic)."""
    k = np.asarray(keys, dtype=np.uint64)
    m = int(mult)
    mask = np.uint64(0xFFFFFFFF)
    a_lo, a_hi = k & mask, k >> np.uint64(32)
    b_lo, b_hi = np.uint64(m & 0xFFFFFFFF), np.uint64(m >> 32)
    ll = a_lo * b_lo
    lh = a_lo * b_hi
    hl = a_hi * b_lo
    hh = a_hi * b_hi
    mid = (ll >> np.uint64(32)) + (lh & mask) + (hl & mask)
    return hh + (lh >> np.uint64(32)) + (hl >> np.uint64(32)) + (mid >> np.uint64(32))


def hand_buckets(keys: np.ndarray, nb: int, maxkey: int | None = None) -> np.ndarray:
    keys = np.asarray(keys, dtype=np.uint64)
    if maxkey is None:
        maxkey = int(keys.max()) if keys.size else 0
    mult, ident = hand_mult(maxkey, nb)
    if ident:
        return np.minimum(keys, np.uint64(nb - 1)).astype(np.int64)
    return _umulhi(keys, mult).astype(np.int64)


def seg_cap(n: int, nb: int) -> int:
    """Places per bucket of the segment partition (a multiple of 64)."""
    mean = int(n) // int(nb) + 1
    return (mean + mean // 2 + 128 + 63) & ~63


# ---- the library partition -----------------------------------------------------------------------------------------
def key_bits(maxkey: int) -> int:
    bits = 1
    while bits < 64 and (int(maxkey) >> bits):
        bits += 1
    return bits


def lib_pb(nw: int, kbits: int):
    """(pb, topbit) of the library partition's bucket grouping; pb = 0: the sort path (fewer than 4 096 entries)."""
    topbit = min(int(kbits), 63)
    if nw < 4096:
        return 0, topbit
    pb = 1
    while (int(nw) >> pb) > HB_MEAN:
        pb += 1
    return (0 if pb > topbit else pb), topbit


def lib_buckets(keys: np.ndarray, pb: int, topbit: int) -> np.ndarray:
    keys = np.asarray(keys, dtype=np.uint64)
    return ((keys >> np.uint64(topbit - pb)) & np.uint64((1 << pb) - 1)).astype(np.int64)


def bucket_sizes(buckets: np.ndarray, nb: int) -> np.ndarray:
    return np.bincount(np.asarray(buckets, dtype=np.int64), minlength=int(nb))


# ---- inputs --------------------------------------------------------------------------------------------------------
class Built:
    """Sketches as runs per source, plus what the construction promises."""

    def __init__(self, n_sources):
        self.runs = [[] for _ in range(n_sources)]
        self.ptr = 0

    def hold(self, key: int, h: int):
        """Key held by h consecutive sources (round robin: never twice by one source)."""
        n = len(self.runs)
        assert h <= n
        for q in range(h):
            self.runs[(self.ptr + q) % n].append(int(key))
        self.ptr = (self.ptr + h) % n

    def arrays(self):
        rs = [np.unique(np.asarray(r, dtype=np.uint64)) for r in self.runs]
        assert sum(r.size for r in rs) == sum(len(r) for r in self.runs), "a source holds a key twice"
        offsets = np.zeros(len(rs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([r.size for r in rs])
        keys = np.concatenate(rs).astype(np.uint64) if rs else np.zeros(0, np.uint64)
        return keys, offsets


def _spread(b: Built, keys, entries: int, per: int):
    """`entries` entries over keys taken from the iterator, `per` holders each (the last key takes the rest)."""
    while entries > 0:
        h = min(per, entries)
        b.hold(next(keys), h)
        entries -= h


def bucket_input(size: int, filler: int, n_sources: int, kind: str = "mixed", rng=None, per: int = 8):
    """One bucket of exactly `size` entries at the top of the key range (its keys have the top 40 bits set, the
    all-ones key among them, so it is the last bucket of either partition), and `filler` entries in keys whose bit 62
    is clear, half with the top bit set: under the hand-written partition at 4 buckets they fill buckets 0 and 2; under
    the library partition they never reach its last bucket (bit 63 is folded away there).
    kind: "mixed" - one key held by every source, the all-ones key by 3, the rest `per` holders a key;
          "pairs" - size / 2 keys of two holders (the all-ones key one of them);
          "one"   - the all-ones key held by `size` sources;
          "distinct:D" - D distinct keys besides the all-ones key (which has a table slot of its own in the bucket
                         kernels, so it is not one of the keys their tables count): one held by size - D sources, the
                         others and the all-ones key by one source each."""
    rng = rng if rng is not None else np.random.default_rng(size * 7 + filler)
    b = Built(n_sources)
    top = iter(range(M64 - 1, M64 - (1 << 40), -1))
    if kind == "mixed":
        b.hold(ALL_ONES, 3)
        b.hold(next(top), n_sources)
        _spread(b, top, size - 3 - n_sources, per)
    elif kind == "pairs":
        assert size % 2 == 0
        b.hold(ALL_ONES, 2)
        _spread(b, top, size - 2, 2)
    elif kind == "one":
        b.hold(ALL_ONES, size)
    elif kind.startswith("distinct:"):
        d = int(kind.split(":")[1])
        b.hold(ALL_ONES, 1)
        b.hold(next(top), size - d)
        _spread(b, top, d - 1, 1)
    else:
        raise ValueError(kind)
    lo = np.unique(rng.integers(1, 1 << 62, size=2 * filler + 16, dtype=np.uint64))
    rng.shuffle(lo)
    h = (filler + 1) // 2
    _spread(b, iter([int(v) for v in lo[:h]]), h, per)                        # top bits 00: bucket 0 of 4
    _spread(b, iter([(2 << 62) | int(v) for v in lo[h:filler]]), filler - h, per)   # top bits 10: bucket 2 of 4
    return b.arrays()


def pair_input(k: int, n_sources: int, a: int, bsrc: int, first_key: int = 1):
    """Sources a and bsrc both hold keys first_key .. first_key + k - 1 (and nothing else is held by anyone)."""
    runs = [np.zeros(0, np.uint64) for _ in range(n_sources)]
    shared = np.arange(first_key, first_key + k, dtype=np.uint64)
    runs[a] = shared
    runs[bsrc] = shared
    offsets = np.zeros(n_sources + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in runs])
    return np.concatenate(runs), offsets

"""The containment columns restated exactly (tests only), and an edge list built to sit where counts stop being exact floats.

A float32 is its BIT PATTERN (a Python int) throughout the exact part of this file: no value is negative, so the patterns
of the numbers order like the numbers, +inf is 0x7F800000 and every NaN is NAN.  The arithmetic is integers and
fractions.Fraction only; as_f32() turns patterns into a numpy array for the callers that compare with numpy or the device.

    f32_of_int, f32_div      the two roundings of src/pairwise.cpp:260-264: (float)count, (float)shared, float / float
    column                   columns 3 (min), 4 (avg), 5 (max) of a record, with the NaN asymmetry of std::min / std::max
    critical_cc / _repr      the smallest float the text test of `kSpider cluster` / of `repr_sketches` lets through, found
                             by bisection over the patterns through the '%.6g' text of each (no call into the product)
    WRONG                    seven deliberately wrong column functions in numpy, for the sensitivity proof of
                             tests/test_exact_values_cpu.py
    hostile_edges            the record list of tests/test_big_counts_gpu.py
    hostile_index            the colour index of its drop-in tests"""
import functools
import struct
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import repr_restate as rr

NAN = 0x7FC00000
INF = 0x7F800000
CUT_CHUNK_EDGES = 2048          # kspider_amd.engine.CUT_CHUNK_EDGES (every chunked pass uses it); asserted equal by the CPU test


# ---- exact float32 arithmetic on bit patterns ----------------------------------------------------------------------------------

def _round(q: Fraction) -> int:
    """The pattern of the float32 nearest to the rational q >= 0, ties to even."""
    if q == 0:
        return 0
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()                      # 2^(e-1) < q < 2^(e+1)
    if (n < (d << e)) if e >= 0 else ((n << -e) < d):
        e -= 1                                               # 2^e <= q < 2^(e+1)
    sub = e < -126
    scale = (-126 if sub else e) - 23                        # q = m x 2^scale, m in [2^23, 2^24) (below 2^23: a subnormal)
    num, den = (n, d << scale) if scale >= 0 else (n << -scale, d)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    if sub:
        return m                                             # (m == 2^23 is the smallest normal: the same pattern)
    if m == 1 << 24:
        m, e = 1 << 23, e + 1
    if e > 127:
        return INF
    return ((e + 127) << 23) | (m - (1 << 23))


def frac(bits: int) -> Fraction:
    """The rational a finite pattern stands for."""
    exp, man = bits >> 23, bits & 0x7FFFFF
    assert 0 <= bits < INF
    if exp == 0:
        return Fraction(man, 1 << 149)
    m, e = man | (1 << 23), exp - 150
    return Fraction(m << e) if e >= 0 else Fraction(m, 1 << -e)


def is_nan(bits: int) -> bool:
    return bits > INF


def f32_of_int(v: int) -> int:
    assert 0 <= v < 1 << 64
    return _round(Fraction(v))


def f32_div(a: int, b: int) -> int:
    """a / b correctly rounded: 0 / 0 and inf / inf are NaN, x / 0 is +inf."""
    if is_nan(a) or is_nan(b):
        return NAN
    if a == INF:
        return NAN if b == INF else INF
    if b == INF:
        return 0
    if b == 0:
        return NAN if a == 0 else INF
    return _round(frac(a) / frac(b))


def f32_add(a: int, b: int) -> int:
    if is_nan(a) or is_nan(b):
        return NAN
    if a == INF or b == INF:
        return INF
    return _round(frac(a) + frac(b))


def _half_through_double(s: int) -> int:
    """(float)((double)s / 2.0): the double holds s / 2 exactly, so this is one rounding of s / 2."""
    if is_nan(s) or s == INF:
        return s
    return _round(frac(s) / 2)


def quotients(shared: int, n1: int, n2: int) -> tuple:
    """(c12, c21) = (shared / n2, shared / n1), every operand rounded to float32 first."""
    sh = f32_of_int(shared)
    return f32_div(sh, f32_of_int(n2)), f32_div(sh, f32_of_int(n1))


def _less(a: int, b: int) -> bool:
    return not is_nan(a) and not is_nan(b) and a < b


def column(shared: int, n1: int, n2: int, col: int) -> int:
    c12, c21 = quotients(shared, n1, n2)
    if col == 3:
        return c21 if _less(c21, c12) else c12               # std::min(c12, c21): a NaN c12 wins, a NaN c21 loses
    if col == 5:
        return c21 if _less(c12, c21) else c12               # std::max(c12, c21)
    assert col == 4
    return _half_through_double(f32_add(c12, c21))


def as_float(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", NAN if is_nan(bits) else bits))[0]


def as_f32(patterns) -> np.ndarray:
    return np.array(patterns, dtype=np.uint32).view(np.float32)


def bits_of(values) -> np.ndarray:
    """The patterns of a float32 array, every NaN as NAN."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    b = v.view(np.uint32).copy()
    b[np.isnan(v)] = NAN
    return b


def text(bits: int) -> str:
    """What the pairwise writer prints: '%.6g' of the float as a double."""
    return "%.6g" % as_float(bits)


def columns(edges: np.ndarray, kmer_counts, col: int) -> list:
    """The patterns of column col of every record."""
    cnt = np.asarray(kmer_counts).tolist()
    return [column(s, cnt[a], cnt[b], col) for a, b, s in zip(edges["source_1"].tolist(), edges["source_2"].tolist(), edges["shared"].tolist())]


def _bisect(passes) -> int | None:
    """The smallest pattern in [0, INF] that passes a test which is monotone in the float; None: not even +inf passes."""
    if passes(0):
        return 0
    if not passes(INF):
        return None
    lo, hi = 0, INF                                          # lo fails, hi passes
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if passes(mid) else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def critical_cc(cutoff: float) -> int | None:
    """ks_clustering.py:101-105: text -> Python float -> x 100 -> not below cutoff x 100."""
    return _bisect(lambda b: not (float(text(b)) * 100 < cutoff * 100))


@functools.lru_cache(maxsize=None)
def critical_repr(threshold: float) -> int | None:
    """apps/repr_sketches.cpp: stof(text) > threshold, the float promoted to double."""
    return _bisect(lambda b: rr.strtof(text(b)) > threshold)


# ---- deliberately wrong columns (numpy), for the sensitivity proof -------------------------------------------------------------

def _combine(c12, c21, col):
    if col == 3:
        return np.where(c21 < c12, c21, c12)
    if col == 5:
        return np.where(c12 < c21, c21, c12)
    return ((c12 + c21).astype(np.float64) / 2.0).astype(np.float32)


def _parts(edges, kmer_counts):
    cnt = np.asarray(kmer_counts)
    return edges["shared"], cnt[edges["source_1"]], cnt[edges["source_2"]]


def _toward_zero(v) -> np.ndarray:
    """float32 of unsigned integers, the bits below the 24 leading ones dropped."""
    return np.array([x & ~((1 << max(0, x.bit_length() - 24)) - 1) for x in np.asarray(v).tolist()], dtype=np.uint64).astype(np.float32)


def _wrong(name):
    def values(edges, kmer_counts, col):
        sh, n1, n2 = _parts(edges, kmer_counts)
        f32 = lambda v: v.astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if name == "shared_through_double":
                c12, c21 = f32(sh.astype(np.float64)) / f32(n2), f32(sh.astype(np.float64)) / f32(n1)
            elif name == "shared_32_bits":
                lo = sh & np.uint64(0xFFFFFFFF)
                c12, c21 = f32(lo) / f32(n2), f32(lo) / f32(n1)
            elif name == "toward_zero":
                c12, c21 = _toward_zero(sh) / _toward_zero(n2), _toward_zero(sh) / _toward_zero(n1)
            elif name == "reciprocal":
                c12, c21 = f32(sh) * (np.float32(1) / f32(n2)), f32(sh) * (np.float32(1) / f32(n1))
            elif name == "double_division":
                c12, c21 = f32(sh.astype(np.float64) / n2.astype(np.float64)), f32(sh.astype(np.float64) / n1.astype(np.float64))
            else:
                c12, c21 = f32(sh) / f32(n2), f32(sh) / f32(n1)
            if name == "double_average" and col == 4:
                return ((c12.astype(np.float64) + c21.astype(np.float64)) / 2.0).astype(np.float32)
            if name == "fmin_fmax" and col in (3, 5):
                return (np.fmin if col == 3 else np.fmax)(c12, c21)
            return _combine(c12, c21, col)
    values.__name__ = name
    return values


# shared converted through a double; shared narrowed to 32 bits; conversions toward zero; a reciprocal-multiply for the quotient; one
# double division of the integers; the average in double without the float rounding of the sum; fminf / fmaxf for std::min / std::max
WRONG = {n: _wrong(n) for n in ("shared_through_double", "shared_32_bits", "toward_zero", "reciprocal", "double_division",
                                "double_average", "fmin_fmax")}


# ---- the hostile record list ---------------------------------------------------------------------------------------------------

EDGE_DTYPE = np.dtype([("source_1", "<u4"), ("source_2", "<u4"), ("shared", "<u8")])
NAMED_COUNTS = (2**24 + 1, 2**24 + 3, 2**25 + 2, 2**31 + 2**7, 2**32 - 1)
EXACT_COUNTS = (1, 7, 2**24, 0)
NAMED_SHARED = (2**32 - 1, 2**32, 2**32 + 1, 2**40 + 2**16, 2**63 + 2**39 + 1, 2**64 - 1)
CUTOFFS = (0.2, 0.25, 0.5, 0.95)
REPR_THRESHOLDS = (0.2, 0.5)
PER_BOUNDARY = 34               # records planted per (column, boundary float); the floor the CPU test asserts is 32
PAIRS_PER_COLUMN = 12           # forest pairs of either kind per column: 36 of each, the floor is 32
ANI_TIES = tuple(range(13, 128, 6))      # odd n: n / 128 has seven decimals ending in 5, a tie at six digits (13 / 128 = 0.1015625)


@dataclass
class Hostile:
    edges: np.ndarray
    kmer_counts: np.ndarray
    cutoffs: list                   # CUTOFFS and the printed value of the row `printed_row`
    printed_row: int
    from_join: np.ndarray           # False: shared >= 2^32, a record only the record-taking entry points can see
    tags: list                      # per record: None, or (kind, number, column) of a forest pair ("same" / "ulp" / "double")
    nan_rows: np.ndarray = field(default=None)      # a NaN in columns 3 and 5 (c12 is one): the rows the ANI calls refuse


def boundaries(cutoffs) -> list:
    """The distinct boundary floats of the list: per cut-off and repr threshold the critical pattern and the one before it."""
    crit = [critical_cc(c) for c in cutoffs] + [critical_repr(t) for t in REPR_THRESHOLDS]
    return sorted({b for c in crit for b in (c, c - 1)})


def find_shared(n1: int, n2: int, col: int, target: int, inexact: bool = True) -> int | None:
    """A shared count whose column col over counts (n1, n2) is exactly `target`, or None; with `inexact` one that is no float
    itself where the rounding interval has room for it."""
    f1, f2 = frac(f32_of_int(n1)), frac(f32_of_int(n2))
    t = frac(target)
    if f1 == 0 or f2 == 0 or t == 0:
        return None
    guess = t * (max(f1, f2) if col == 3 else min(f1, f2) if col == 5 else 2 / (1 / f1 + 1 / f2))
    if not 1 <= guess < 1 << 64:
        return None
    mid = f32_of_int(min(round(guess), (1 << 64) - 1))
    for g in (mid, mid - 1, mid + 1, mid - 2, mid + 2, mid - 3, mid + 3):
        if g >= INF or frac(g).denominator != 1:
            continue
        s = int(frac(g))
        if not 1 <= s < 1 << 64 or column(s, n1, n2, col) != target:
            continue
        if inexact and s + 1 < 1 << 64 and f32_of_int(s + 1) == g:
            return s + 1
        return s
    return None


class _Build:
    def __init__(self, rng):
        self.rng = rng
        self.counts = []
        self.rec = []                    # (node, node, shared, tag)

    def node(self, count: int) -> int:
        self.counts.append(int(count))
        return len(self.counts) - 1

    def odd(self, lo=1 << 24, hi=1 << 32) -> int:
        return int(self.rng.integers(lo, hi)) | 1

    def add(self, a, b, shared, tag=None):
        assert a != b and 0 <= shared < 1 << 64
        self.rec.append((a, b, int(shared), tag))

    def pick(self, pool):
        return pool[int(self.rng.integers(0, len(pool)))]

    def pair(self, pool, apart: bool):
        """Two nodes of the pool; with `apart` their counts differ by a fifth at least."""
        while True:
            a, b = self.pick(pool), self.pick(pool)
            lo, hi = sorted((self.counts[a], self.counts[b]))
            if a != b and (not apart or 5 * lo <= 4 * hi):
                return a, b


def _double_rounding_row(B, big):
    """(m, c): shared = (m << 40) + 2^39 + 1 rounds up to (m + 1) << 40, and down through a double; over equal counts c the value
    is the critical float of its own printed text, and the value of the numerator rounded down is the float before it."""
    while True:
        m = (int(B.rng.integers(1 << 23, (1 << 23) + (1 << 20))) >> 1) << 1
        c = B.counts[B.pick(big)]
        s = (m << 40) + (1 << 39) + 1
        up = f32_of_int(s)
        assert frac(up) == (m + 1) << 40
        v, low = f32_div(up, f32_of_int(c)), f32_div(up - 1, f32_of_int(c))
        if low == v - 1 and text(low) != text(v) and critical_cc(float(text(v))) == v:
            return m, c


@functools.lru_cache(maxsize=None)
def hostile_edges(seed: int = 1) -> Hostile:
    rng = np.random.default_rng([seed, 24])
    B = _Build(rng)
    named = [B.node(c) for c in NAMED_COUNTS + (2**25 + 2, 2**25 + 2)]
    exact = [B.node(c) for c in EXACT_COUNTS[:3]]
    zeros = [B.node(0) for _ in range(4)]
    big = [B.node(B.odd(1 << 31)) for _ in range(40)]                       # above 2^31: a float is a multiple of 256 there
    rnd = [B.node(B.odd()) for _ in range(380)]
    core = named + big + rnd                                                 # every count inexact

    # the row whose printed value is the fifth cut-off, and the forest pair that a conversion through a double reorders
    m, c = _double_rounding_row(B, big)
    hub = B.node(c)
    core.append(hub)
    printed_shared = (m << 40) + (1 << 39) + 1
    B.add(B.node(c), hub, printed_shared, ("double", 0, 5))
    B.add(B.node(c), hub, (m + 1) << 40, ("double", 0, 5))
    cutoffs = list(CUTOFFS) + [float(text(column(printed_shared, c, c, 5)))]

    # boundary rows: per column and boundary float, over nodes with inexact counts
    for col in (3, 4, 5):
        for target in boundaries(cutoffs):
            found = 0
            while found < PER_BOUNDARY:
                a, b = B.pair(core, apart=col != 4)
                s = find_shared(B.counts[a], B.counts[b], col, target)
                if s is not None:
                    B.add(a, b, s)
                    found += 1

    # forest pairs: every record the only connection of a leaf of its own
    for col in (3, 4, 5):
        for kind in ("same", "ulp"):
            made = 0
            while made < PAIRS_PER_COLUMN:
                h1, h2 = B.pick(core), B.pick(core)
                l1, l2 = B.odd(), B.odd()
                s1 = int(rng.integers(1, min(l1, B.counts[h1])))
                target = column(s1, l1, B.counts[h1], col) + (kind == "ulp")
                s2 = find_shared(l2, B.counts[h2], col, target)
                if s2 is None or (s1, l1, B.counts[h1]) == (s2, l2, B.counts[h2]):
                    continue
                B.add(B.node(l1), h1, s1, (kind, made, col))
                B.add(B.node(l2), h2, s2, (kind, made, col))
                made += 1

    # NaN and inf rows, among the core and as the only connection of a leaf
    for z in zeros:
        for _ in range(3):
            B.add(z, B.pick(core), 0)
            B.add(z, B.pick(core), B.pick([1, 2**24 + 1, 2**32 - 1]))
    B.add(zeros[0], zeros[1], 0)
    B.add(zeros[2], zeros[3], 5)
    for _ in range(10):
        B.add(B.node(0), B.pick(core), 0)
    for _ in range(4):
        B.add(B.node(0), B.pick(core), 3)
        B.add(B.node(B.odd()), B.pick(zeros), 0)

    # the named shared counts, and the exact counts
    for s in NAMED_SHARED:
        for _ in range(3):
            a, b = B.pair(core, apart=False)
            B.add(a, b, s)
    for e in exact:
        for _ in range(4):
            B.add(e, B.pick(core), int(rng.integers(0, B.counts[e] + 1)))
    B.add(exact[0], exact[1], 1)

    # ANI rows: six-digit ties over counts that round to 2^25, and values next to 0.0001 and 0.9999 over counts above 2^31
    for n in ANI_TIES:
        B.add(named[2], named[5 + n // 6 % 2], n << 18)
    for edge in (Fraction(1, 10000), Fraction(9999, 10000)):
        for _ in range(16):
            a, b = B.pair(big, apart=False)
            f = frac(f32_of_int(B.counts[a if rng.random() < 0.5 else b]))
            width = max(2, int(60 * edge * f) >> 24)                         # some 60 ulps of the value, in units of shared
            B.add(a, b, round(edge * f) + int(rng.integers(-width, width + 1)))

    # the rest: random pairs of the core, shared not above the smaller count; a third of them inexact floats above 2^24
    total = 3 * CUT_CHUNK_EDGES + 17
    assert len(B.rec) < total - 1500, len(B.rec)
    while len(B.rec) < total:
        a, b = B.pair(core, apart=False)
        lo = min(B.counts[a], B.counts[b])
        kind = int(rng.integers(0, 3))
        s = int(rng.integers(0, lo + 1)) if kind == 0 else int(lo * rng.uniform(0.1, 0.7)) if kind == 1 else (int(rng.integers(1 << 24, lo + 1)) | 1)
        B.add(a, b, s)

    # node numbers and record order at random; every record with source_1 < source_2; the first record of a pair first
    number = rng.permutation(len(B.counts))
    counts = np.zeros(len(B.counts), dtype=np.uint32)
    counts[number] = B.counts
    order = rng.permutation(total).tolist()
    first, second = sorted(pos for pos, i in enumerate(order) if B.rec[i][3] and B.rec[i][3][0] == "double")
    if B.rec[order[first]][2] != printed_shared:                             # the one that rounds differently through a double comes first
        order[first], order[second] = order[second], order[first]
    edges = np.zeros(total, dtype=EDGE_DTYPE)
    tags = []
    for pos, i in enumerate(order):
        a, b, s, tag = B.rec[i]
        a, b = sorted((int(number[a]), int(number[b])))
        edges[pos] = (a, b, s)
        tags.append(tag)
    printed = next(i for i in range(total) if int(edges["shared"][i]) == printed_shared)
    nan = np.array([is_nan(column(s, int(counts[a]), int(counts[b]), 3)) or is_nan(column(s, int(counts[a]), int(counts[b]), 5))
                    for a, b, s in zip(edges["source_1"].tolist(), edges["source_2"].tolist(), edges["shared"].tolist())], dtype=bool)
    return Hostile(edges=edges, kmer_counts=counts, cutoffs=cutoffs, printed_row=printed, from_join=edges["shared"] < np.uint64(1 << 32),
                   tags=tags, nan_rows=nan)


# ---- the hostile colour index --------------------------------------------------------------------------------------------------

INDEX_SOURCES = 40
INDEX_BASE = 2**24 + 1          # the weight of the colour that holds every source: no pair shares less


@functools.lru_cache(maxsize=None)
def hostile_index(seed: int = 1) -> dict:
    """A colour index for oracle.write_index: 40 sources (ids 1 .. 40), every count an inexact float above 2^24 (2^32 - 1 and
    2^31 + 2^7 among them), 300 random colours of weights near 2^22 over the first 28 sources, so that shared lands in (2^24, 2^32),
    and six pairs of the other twelve whose own colour is weighed so that one column of their row is the critical float of the
    cut-off 0.2 or the float before it ("boundary": (id_1, id_2, column, pattern))."""
    rng = np.random.default_rng([seed, 25])
    n_rand = 28
    colours = [(list(range(1, INDEX_SOURCES + 1)), INDEX_BASE)]
    for _ in range(300):
        size = int(rng.integers(2, 6))
        colours.append((sorted(int(x) for x in rng.choice(np.arange(1, n_rand + 1), size=size, replace=False)), int(rng.integers(1 << 18, 1 << 24)) | 1))
    counts = {g: int(rng.integers(1 << 30, 1 << 32)) | 1 for g in range(1, n_rand + 1)}
    counts[3], counts[17] = 2**32 - 1, 2**31 + 2**7
    boundary, g = [], n_rand + 1
    crit = critical_cc(0.2)
    for col in (3, 4, 5):
        for target in (crit, crit - 1):
            while True:
                na, nb = int(rng.integers(1 << 27, 1 << 32)) | 1, int(rng.integers(1 << 27, 1 << 32)) | 1
                if 5 * min(na, nb) > 4 * max(na, nb):
                    continue
                s = find_shared(na, nb, col, target)
                if s is not None and INDEX_BASE < s < 2**32 - INDEX_BASE:
                    break
            counts[g], counts[g + 1] = na, nb
            colours.append(([g, g + 1], s - INDEX_BASE))
            boundary.append((g, g + 1, col, target))
            g += 2
    assert g == INDEX_SOURCES + 1
    order = rng.permutation(len(colours))
    off, src, w = [0], [], []
    for i in order:
        members, weight = colours[int(i)]
        src += [int(x) for x in rng.permutation(members)]
        off.append(len(src))
        w.append(weight)
    gids = [int(x) for x in rng.permutation(sorted(counts))]
    return dict(color_off=np.array(off, dtype=np.uint32), sources=np.array(src, dtype=np.uint32), color_w=np.array(w, dtype=np.uint32),
                group_ids=np.array(gids, dtype=np.uint32), kmer_counts=np.array([counts[x] for x in gids], dtype=np.uint32),
                n_names=INDEX_SOURCES, boundary=boundary)

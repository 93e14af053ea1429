"""Inputs of the device's row text and its restatement on the host, shared by tests/test_tsv_cpu.py (which checks
what the inputs are said to be, without a GPU) and tests/test_tsv_gpu.py.

The yardstick is the project's host definition and never the device's own output: engine.format_float — the host's snprintf
"%.6g", here through engine.format_floats, the same call on many values at once — for a float's text, and the numpy float32
column maths of tests/repr_restate.py for the three containments."""
from fractions import Fraction

import numpy as np

import repr_restate as rr
from kspider_amd import engine

EDGE_DTYPE = engine.EDGE_DTYPE
C = engine.TSV_CHUNK_ROWS
ROW_MIN, ROW_MAX = engine.TSV_ROW_MIN, engine.TSV_ROW_MAX
LO, HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)        # the finite positive domain is [LO, HI)
#: rows(n) for these n: around a wave, around a chunk (one row per lane of 256), and several chunks with a ragged end
ROW_COUNTS = sorted({0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 17})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def float_texts(values) -> list:
    """engine.format_float of every value; each distinct bit pattern is formatted once."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    bits, inverse = np.unique(v.view(np.uint32), return_inverse=True)
    texts = np.array(engine.format_floats(bits.view(np.float32)), dtype=object)
    return texts[inverse].tolist()


def rows_text(edges, counts, ids=None) -> bytes:
    """The rows of the pairwise TSV for these records, without the header: id1, id2, shared and the writer's three float32
    containments, each as engine.format_float prints it."""
    if len(edges) == 0:
        return b""
    counts = np.asarray(counts, dtype=np.uint32)
    a, b = edges["source_1"], edges["source_2"]
    id1, id2 = (a, b) if ids is None else (np.asarray(ids)[a], np.asarray(ids)[b])
    cols = [float_texts(rr.column_values(edges, counts, col)) for col in (3, 4, 5)]
    return "".join(f"{x}\t{y}\t{s}\t{mn}\t{av}\t{mx}\n" for x, y, s, mn, av, mx in
                   zip(id1.tolist(), id2.tolist(), edges["shared"].tolist(), *cols)).encode()


def edges(s1, s2, shared):
    e = np.zeros(len(s1), dtype=EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = s1, s2, shared
    return e


# ---- floats ------------------------------------------------------------------------------------------------------------------------

def in_domain(v):
    v = np.asarray(v, dtype=np.float32)
    return v[(v >= LO) & (v < HI)]


def powers_of_two():
    return np.array([2.0 ** k for k in range(-40, 40)], dtype=np.float32)


def small_multiples():
    """j * 2^k for j < 4096 and every k that leaves a value in the domain."""
    j = np.arange(1, 4096, dtype=np.float64)
    return np.unique(in_domain(np.concatenate([j * 2.0 ** k for k in range(-52, 40)])))


def quotients(n_max=4096):
    """s / n in float32 for 1 <= s <= n <= n_max: what a containment of small sketches looks like."""
    out = [np.arange(1, n + 1, dtype=np.float32) / np.float32(n) for n in range(1, n_max + 1)]
    return np.unique(np.concatenate(out))


def exact(v) -> Fraction:
    return Fraction(float(np.float32(v)))


def around(boundary: Fraction):
    """(the largest float32 below the boundary, the smallest float32 at or above it)"""
    f = np.float32(float(boundary))
    while exact(f) >= boundary:
        f = np.nextafter(f, np.float32(0))
    while exact(np.nextafter(f, np.float32(np.inf))) < boundary:
        f = np.nextafter(f, np.float32(np.inf))
    return f, np.nextafter(f, np.float32(np.inf))


DECADES = range(-12, 13)
NOTATION_SWITCHES = (-5, -4, 5, 6)          # 1e-05 | 0.0001 and 100000 | 1e+06: where %g changes between scientific and fixed


def decade_neighbours():
    """{X: (below, at_or_above)} of 10^X."""
    return {X: around(Fraction(10) ** X) for X in DECADES}


def carry_neighbours():
    """{X: (below, at_or_above)} of 9.999995 * 10^(X - 1): below it six nines are printed, from it on the digits carry into 10^X."""
    return {X: around(Fraction(9999995, 1000000) * Fraction(10) ** (X - 1)) for X in DECADES}


#: (value, its text): the seventh significant digit of the exact value is a 5 with nothing behind it.  "even": the sixth digit is
#: even and stays; "up": it is odd and goes up.
TIES = {
    "even": [(1 / 1024, "0.000976562"), (1 / 512, "0.00195312"), (5 / 512, "0.00976562"), (100000.5, "100000"), (1000005.0, "1e+06")],
    "up": [(3 / 512, "0.00585938"), (3 / 256, "0.0117188"), (100001.5, "100002"), (1000015.0, "1.00002e+06"), (7 / 256, "0.0273438")],
}


def ties():
    return np.array([v for kind in TIES.values() for v, _ in kind], dtype=np.float32)


def random_floats(n=1 << 20, seed=20261019):
    """n bit patterns of the finite positive domain: every binary exponent from -40 to 39 with a random significand."""
    rng = np.random.default_rng(seed)
    bits = (rng.integers(127 - 40, 127 + 40, size=n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, size=n, dtype=np.uint32)
    return bits.astype(np.uint32).view(np.float32)


#: outside the domain: a denormal, 2^40, a negative number, a NaN
REFUSED = [np.float32(1e-40), np.float32(2.0 ** 40), np.float32(-1.0), np.float32(np.nan)]


# ---- rows --------------------------------------------------------------------------------------------------------------------------

N_NODES = 1000


def node_tables(seed=5):
    """(counts, ids) of N_NODES nodes: 40 distinct k-mer counts of 1 to 10 digits, and a permuted id table of 1 to 10 digits."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[1, 2, 7, 4294967295], (10.0 ** rng.uniform(0, 9.6, size=36)).astype(np.uint64)])).astype(np.uint32)
    counts = pool[rng.integers(0, len(pool), size=N_NODES)]
    ids = np.unique((10.0 ** rng.uniform(0, 9.63, size=4 * N_NODES)).astype(np.uint64))
    ids = ids[ids < (1 << 32)]
    ids = rng.permutation(ids)[:N_NODES].astype(np.uint32)
    return counts, ids


def rows(n, seed=1):
    """n records over node_tables(): shared counts of 1 to 12 digits from a pool of 50 (every column stays below 2^40), ends at
    random, in no order."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[1, 9, 10, 999999999999], (10.0 ** rng.uniform(0, 11.9, size=46)).astype(np.uint64)]))
    return edges(rng.integers(0, N_NODES, size=n), rng.integers(0, N_NODES, size=n), pool[rng.integers(0, len(pool), size=n)])


def extreme_tables():
    """(counts, ids) for shortest_rows / longest_rows: nodes 0 .. 9 have one-digit ids and 7 k-mers, the nodes behind them ten-digit
    ids and counts near 2^32."""
    counts = np.concatenate([np.full(10, 7), 4294967295 - 1024 * np.arange(N_NODES - 10)]).astype(np.uint32)
    ids = np.concatenate([np.arange(10), 4294967295 - np.arange(N_NODES - 10)]).astype(np.uint32)
    return counts, ids


def shortest_rows(n):
    """n rows of ROW_MIN bytes: one-digit ids, shared = 7 = both counts, so every column is 1."""
    i = np.arange(n)
    return edges(i % 10, (i + 3) % 10, np.full(n, 7))


def longest_rows(n):
    """n rows of ROW_MAX bytes: ten-digit ids, a shared count of 20 digits, three floats in scientific notation with six digits."""
    i = np.arange(n, dtype=np.uint64)
    shared = np.uint64(10 ** 19) + i * np.uint64(7 * 10 ** 15 + 1)
    e = edges(10 + (i % 400), 500 + (i * 7 % 400), shared)
    counts, ids = extreme_tables()
    keep = np.array([len(r) == ROW_MAX - 1 for r in rows_text(e, counts, ids).decode().split("\n")[:-1]])
    return e, keep


def longest_only(n):
    """n rows, every one ROW_MAX bytes long."""
    e, keep = longest_rows(2 * n)
    assert keep.sum() >= n
    return e[keep][:n]


def alternating_rows(n):
    e = np.zeros(n, dtype=EDGE_DTYPE)
    e[0::2] = shortest_rows(len(e[0::2]))
    e[1::2] = longest_only(len(e[1::2]))
    return e


def inf_rows():
    """(edges, counts): sources of 0 k-mers beside shared > 0: +inf in one, two or all three columns; and shared = 0 beside
    counts > 0: three zeros."""
    counts = np.array([0, 0, 5, 10, 3], dtype=np.uint32)
    return edges([0, 0, 1, 2, 2, 3], [1, 2, 3, 3, 4, 4], [4, 5, 6, 5, 0, 0]), counts


def nan_rows():
    """(edges, counts): row 2 has shared = 0 beside a count of 0: a NaN column."""
    counts = np.array([0, 4, 5, 10], dtype=np.uint32)
    return edges([1, 2, 0, 2], [2, 3, 1, 3], [1, 2, 0, 3]), counts

"""A plain-Python restatement of the reference's `repr_sketches` tool (apps/repr_sketches.cpp:27-33,38-43): the
yardstick of tests/test_repr_cpu.py and tests/test_repr_gpu.py.  The tool itself cannot be built here (boost and phmap
are absent), so no reference-generated output pins the ranking: this file restates what its 44 lines do.

    for every data line of the pairwise TSV (header skipped):
        containment = stof(column 4)                 # a C float
        if containment > 0.20:                       # the float promoted to double, strictly
            count[stoi(column 0)] += 1
            count[stoi(column 1)] += 1
    print "id: count" per id with a count, largest count first

The order among equal counts is not pinned there (an unstable sort over a hash map's iteration order); the canonical
order used here and by the product is count descending, then id ascending.

The text is parsed with glibc's strtof through ctypes: numpy.float32(text) parses to a double first and rounds twice.
Nothing in this file uses a critical float: every value goes through its own text."""
import ctypes

import numpy as np

_libc = ctypes.CDLL(None)
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]


def strtof(text: str) -> float:
    """The C float stof makes of `text`, as a Python float (exact)."""
    return _libc.strtof(text.encode(), None)


def text_passes(text: str, threshold: float = 0.20) -> bool:
    return strtof(text) > threshold          # (a NaN is never above anything)


def float_passes(value, threshold: float = 0.20) -> bool:
    """The test on a float32 that the pairwise writer prints with 6 significant digits."""
    return text_passes("%.6g" % float(np.float32(value)), threshold)


def counts(tsv_text: str, col: int = 4, threshold: float = 0.20) -> dict:
    out = {}
    for line in tsv_text.split("\n")[1:]:
        if not line:
            continue
        p = line.split("\t")
        if text_passes(p[col], threshold):
            for c in (0, 1):
                out[int(p[c])] = out.get(int(p[c]), 0) + 1
    return out


def ranked(count: dict) -> list:
    """[(id, count)] in canonical order: count descending, id ascending."""
    return sorted(((k, v) for k, v in count.items() if v), key=lambda kv: (-kv[1], kv[0]))


def render(rank: list) -> bytes:
    return "".join(f"{k}: {v}\n" for k, v in rank).encode()


def repr_sketches(tsv_text: str, col: int = 4, threshold: float = 0.20) -> bytes:
    """What the tool prints for this TSV, in canonical order."""
    return render(ranked(counts(tsv_text, col, threshold)))


def column_values(edges: np.ndarray, kmer_counts: np.ndarray, col: int) -> np.ndarray:
    """Column col (3 min, 4 avg, 5 max) of every edge as the pairwise writer computes it (src/pairwise.cpp:260-264):
    single-precision divisions, std::min / std::max of the two, the average through a double."""
    with np.errstate(divide="ignore", invalid="ignore"):
        sh = edges["shared"].astype(np.float32)
        n1 = kmer_counts[edges["source_1"]].astype(np.float32)
        n2 = kmer_counts[edges["source_2"]].astype(np.float32)
        c12, c21 = sh / n2, sh / n1
        if col == 3:
            return np.where(c21 < c12, c21, c12)       # std::min(c12, c21)
        if col == 5:
            return np.where(c12 < c21, c21, c12)       # std::max(c12, c21)
        return ((c12 + c21).astype(np.float64) / 2.0).astype(np.float32)


def degrees(edges: np.ndarray, kmer_counts: np.ndarray, col: int, threshold: float, n_nodes: int | None = None) -> np.ndarray:
    """Brute force: every edge through its '%.6g' text and strtof; both ends of a passing edge counted."""
    n = len(kmer_counts) if n_nodes is None else n_nodes
    out = np.zeros(n, dtype=np.uint32)
    vals = column_values(edges, kmer_counts, col)
    s1, s2 = edges["source_1"].tolist(), edges["source_2"].tolist()
    for i, v in enumerate(vals.tolist()):
        if strtof("%.6g" % v) > threshold:
            out[s1[i]] += 1
            out[s2[i]] += 1
    return out

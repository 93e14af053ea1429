"""Restatements of how the sliced stage 1 cuts its input (CPU, integers only) and inputs built to sit on those cuts.

Sketch input (engine.hip, build_impl in slice mode): the keys of [0, span) are shared out in key order, span being the
largest key + 1, or 2^key_bits when the caller fixed key_bits.  The contract restated here is a partition: part p holds
the keys span * p // nparts <= k < span * (p + 1) // nparts (an empty range when span < nparts leaves nothing for it).
Postings input (slice_plan.h, the plan of run_multi in multi.hip): whole keys, cut where the memberships reach s / nd of all of them.
"""
import numpy as np

from kspider_amd import engine

M64 = (1 << 64) - 1


# ---- the key-range cut ---------------------------------------------------------------------------------------------
def key_cuts(span: int, nparts: int) -> list:
    """[(lo, end)] per part, end exclusive, Python integers (span up to 2^64)."""
    span, nparts = int(span), int(nparts)
    assert 1 <= span <= 1 << 64 and nparts >= 1
    return [(span * p // nparts, span * (p + 1) // nparts) for p in range(nparts)]


def part_of(keys, span: int, nparts: int) -> np.ndarray:
    """Part of every key (all below span).  Exact for 64-bit keys: the cuts are Python integers, the comparison is one
    of uint64 values (end - 1 of every part whose end is not 0)."""
    keys = np.asarray(keys, dtype=np.uint64)
    ends = [end for _, end in key_cuts(span, nparts)]
    z = sum(1 for end in ends if end == 0)          # leading parts with nothing below their end
    last = np.array([end - 1 for end in ends[z:]], dtype=np.uint64)
    p = z + np.searchsorted(last, keys, side="left")   # first part whose end lies above the key
    assert keys.size == 0 or (int(keys.max()) < span and int(p.max()) < nparts)
    return p.astype(np.int64)


def engine_span(keys, key_bits: int = 0) -> int:
    """The span the engine cuts: largest key + 1, or 2^key_bits when the caller passes key_bits."""
    if key_bits > 0:
        return 1 << key_bits
    keys = np.asarray(keys, dtype=np.uint64)
    return int(keys.max()) + 1 if keys.size else 1


def kept_keys_per_part(keys, span: int, nparts: int) -> np.ndarray:
    """Distinct keys with two holders or more (what stage 1 keeps) in every part: slice_sizes()[1] of that slice."""
    uk, cnt = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    return np.bincount(part_of(uk[cnt >= 2], span, nparts), minlength=nparts)[:nparts]


# ---- the postings cut ----------------------------------------------------------------------------------------------
def postings_cuts(key_off, nparts: int) -> list:
    """Slice s holds the keys [cuts[s], cuts[s + 1]): goal n / nd * s memberships before the cut, whole keys, no empty
    slice, at least one key left for every later slice.  More slices than keys (or one): a single build, [0, n_keys]."""
    key_off = [int(x) for x in np.asarray(key_off).tolist()]
    n_keys, nd = len(key_off) - 1, int(nparts)
    if nd <= 1 or nd > n_keys:
        return [0, n_keys]
    n = key_off[n_keys]
    cuts, k = [0], 0
    for s in range(1, nd):
        goal = n // nd * s
        while k < n_keys and key_off[k] < goal:
            k += 1
        k = max(k, cuts[-1] + 1)
        k = min(k, n_keys - (nd - s))
        cuts.append(k)
    cuts.append(n_keys)
    return cuts


# ---- inputs --------------------------------------------------------------------------------------------------------
def arrays(runs):
    """(keys, offsets) of runs (lists of Python integers, any order, no key twice in a run)."""
    rs = [np.array(sorted(r), dtype=np.uint64) for r in runs]
    assert all(np.unique(r).size == r.size for r in rs), "a source holds a key twice"
    offsets = np.zeros(len(rs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in rs])
    keys = np.concatenate(rs) if rs else np.zeros(0, np.uint64)
    return keys.astype(np.uint64), offsets


def edges_of(rows) -> np.ndarray:
    """{(a, b): shared} or [(a, b, shared)] -> EDGE_DTYPE array in (source_1, source_2) order."""
    if isinstance(rows, dict):
        rows = [(a, b, c) for (a, b), c in rows.items()]
    rows = sorted(rows)
    out = np.zeros(len(rows), dtype=engine.EDGE_DTYPE)
    if rows:
        r = np.array(rows, dtype=np.uint64)
        out["source_1"], out["source_2"], out["shared"] = r[:, 0], r[:, 1], r[:, 2]
    return out


def boundary_keys(span: int, nparts: int) -> list:
    """Per part: its keys lo, lo + 1, end - 2, end - 1 and one in the middle, those that exist, in key order."""
    out = []
    for lo, end in key_cuts(span, nparts):
        ks = {k for k in (lo, lo + 1, end - 2, end - 1, (lo + end) // 2) if lo <= k < end}
        out.append(sorted(ks))
    return out


def cut_input(span: int, nparts: int, n_sources: int = 0, empty_parts=(), singles: int = 3):
    """Sketches on the cuts of [0, span): every boundary key of every part (boundary_keys) is held by exactly one pair
    of sources (2j, 2j + 1), pairs taken round robin, and no two pairs have a key in common: the edge set is
    {(2j, 2j + 1): number of keys given to pair j}.  One misplaced, lost or doubled key changes one named edge.
    n_sources 0: a pair per key.  empty_parts: parts that get no key at all (when the last part is not among them, key
    span - 1 is present and the engine derives this span from the data; otherwise the caller fixes it by key_bits).
    singles: keys next to the middle of a part held by one source each (stage 1 drops them).
    Returns (keys, offsets, edges, kept: distinct shared keys per part)."""
    per_part = boundary_keys(span, nparts)
    for p in empty_parts:
        per_part[p] = []
    flat = [k for ks in per_part for k in ks]
    if n_sources <= 0:
        n_sources = 2 * len(flat)
    npairs = n_sources // 2
    assert npairs >= 1
    runs = [[] for _ in range(n_sources)]
    want = {}
    for i, k in enumerate(flat):
        j = i % npairs
        runs[2 * j].append(k)
        runs[2 * j + 1].append(k)
        want[(2 * j, 2 * j + 1)] = want.get((2 * j, 2 * j + 1), 0) + 1
    used = set(flat)
    s = 0
    for (lo, end), ks in zip(key_cuts(span, nparts), per_part):
        if not ks:
            continue
        for q in range(singles):
            k = (lo + end) // 2 + 1 + q
            if lo <= k < end and k not in used:
                used.add(k)
                runs[s % n_sources].append(k)
                s += 1
    keys, offsets = arrays(runs)
    kept = np.array([len(ks) for ks in per_part], dtype=np.int64)
    return keys, offsets, edges_of(want), kept


def small_span_input(span: int, holders: int = 2, n_sources: int = 0):
    """Keys 0 .. span - 1, key k held by `holders` consecutive sources starting at source k (so neighbouring keys
    overlap in holders - 1 sources).  Returns (keys, offsets, {key: holders' list})."""
    n = n_sources or span + holders - 1
    runs = [[] for _ in range(n)]
    who = {}
    for k in range(span):
        who[k] = [(k + q) % n for q in range(holders)]
        for s in who[k]:
            runs[s].append(k)
    keys, offsets = arrays(runs)
    return keys, offsets, who


def pairs_from_holders(who: dict, weight=None) -> np.ndarray:
    """Edge set of {key: holders}: every pair of holders of a key shares it (weight[key] or 1 per key; sums of 0 are
    not edges)."""
    want = {}
    for k, hs in who.items():
        w = 1 if weight is None else int(weight[k])
        hs = sorted(hs)
        for x in range(len(hs)):
            for y in range(x + 1, len(hs)):
                want[(hs[x], hs[y])] = want.get((hs[x], hs[y]), 0) + w
    return edges_of({p: c for p, c in want.items() if c})

"""Inputs of the compare tests (tests/test_compare_gpu.py, tests/test_compare_files_gpu.py).  A case is (db, q): two lists of
sources, each a dict hash -> abundance.  tests/test_compare_inputs_cpu.py shows that every builder makes the case it is named
for; the expectation is tests/compare_restate.py.  Nothing here calls the code under test."""
import numpy as np

TOP32 = 2**32 - 1
LIMIT_ABUNDS = (4294967295, 92681, 408, 19, 2)   # Σ a² = 2^64 - 1; with 3 for the 2: 2^64 + 4


def arrays(sources, counted=True):
    """(keys, abund or None, offsets) of a side: the runs ascending, back to back; counted False: no abundance array"""
    keys, abund, offsets = [], [], [0]
    for s in sources:
        for h in sorted(s):
            keys.append(h)
            abund.append(s[h])
        offsets.append(len(keys))
    return np.array(keys, dtype=np.uint64), (np.array(abund, dtype=np.uint32) if counted else None), np.array(offsets, dtype=np.uint64)


def flat(sources):
    """the same sources with every abundance 1"""
    return [{h: 1 for h in s} for s in sources]


def hand_case():
    """One database source and three queries: q0 and q1 are the same counted sample, q2 is flat and shares two hashes with them,
    q3 shares nothing with anybody.  By hand, CROSS_AND_SELF, sources d0 = 0, q0 = 1, q1 = 2, q2 = 3, q3 = 4:
      (0, 1): hashes 10, 20      dot 2·3 + 5·1 = 11     mass 7, 4        (0, 2): the same
      (0, 3): hash 20            dot 5·1 = 5            mass 5, 1
      (1, 2): hashes 10, 20, 30  dot 9 + 1 + 16 = 26    mass 8, 8        (identical: cosine 1)
      (1, 3), (2, 3): 20, 30     dot 1 + 4 = 5          mass 5, 2"""
    d0 = {10: 2, 20: 5, 99: 7}
    q0 = {10: 3, 20: 1, 30: 4}
    return [d0], [q0, dict(q0), {20: 1, 30: 1, 40: 1}, {1000: 6, 1001: 1}]


HAND_ROWS = [(0, 1, 2, 11, 7, 4), (0, 2, 2, 11, 7, 4), (0, 3, 1, 5, 5, 1), (1, 2, 3, 26, 8, 8), (1, 3, 2, 5, 5, 2), (2, 3, 2, 5, 5, 2)]
HAND_SUMS = ([14, 8, 8, 3, 7], [78, 26, 26, 3, 37])


def random_case(seed=31, n_db=12, n_q=28, universe=2000, largest=300):
    """40 sources of up to `largest` hashes from a small universe, so that most pairs share some; heavy-tailed abundances (a Pareto
    tail up to a few thousand, most of them 1 or 2)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_db + n_q):
        size = int(rng.integers(1, largest + 1))
        hashes = rng.choice(universe, size=size, replace=False)
        abunds = np.minimum(np.floor(rng.pareto(0.9, size=size)) + 1, 5000).astype(np.int64)
        out.append({int(h) * 0x9E3779B97F4A7C15 % 2**64: int(a) for h, a in zip(hashes, abunds)})
    return out[:n_db], out[n_db:]


def width_case():
    """q0 and q1 share one hash at abundance 2^32 - 1: dot = 2^64 - 2^33 + 1, above 2^63.  q2 and q3 share 40 hashes whose products
    are 3·2^30 each: the running sum crosses 2^32 at the second and 2^33 at the third, and ends at 120·2^30."""
    many = {1000 + i: 3 * 2**15 for i in range(40)}
    return [], [{7: TOP32}, {7: TOP32, 8: 1}, dict(many), {h: 2**15 for h in many}]


def limit_case(last):
    """a source whose abundances are LIMIT_ABUNDS with `last` for the last, and a small flat one that shares its first hash"""
    big = {100 + i: a for i, a in enumerate(LIMIT_ABUNDS[:-1] + (last,))}
    return big, {100: 1, 7: 1}


def seams_case(seed=5, n=1100, universe=6000):
    """1 100 queries of 1 .. 8 hashes: three tiles of 512 by default, and with a tile of 1 or 3 every probing query has tiles in
    front of it, around it and behind it"""
    rng = np.random.default_rng(seed)
    return [], [{int(h) + 1: int(rng.integers(1, 50)) for h in rng.choice(universe, size=int(rng.integers(1, 9)), replace=False)} for _ in range(n)]


def list_case(n=300):
    """300 queries that hold one and the same hash, with abundances 1 .. 300: query 0 touches the 299 others of its tile"""
    return [], [{77: i + 1} for i in range(n)]

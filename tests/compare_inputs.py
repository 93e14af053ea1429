"""Inputs of the compare tests (tests/test_compare_gpu.py, tests/test_compare_edges_gpu.py, tests/test_compare_files_gpu.py).  A case is (db, q): two lists of
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


# ---- the edges (tests/test_compare_edges_gpu.py) ------------------------------------------------------------------------------
def _heavy(rng, size):
    """random_case's abundances"""
    return np.minimum(np.floor(rng.pareto(0.9, size=size)) + 1, 5000).astype(np.int64)


BLOCK_RUN_LENGTHS = (255, 256, 257, 1023, 1024, 1025, 3)
BLOCK_QUERY_LENGTH = 600


def block_case(seed=4, universe=3000):
    """Database runs one short of, exactly and one past what a wave (64 lanes x 4 keys = 256 entries) and a workgroup (1 024) look up
    in one trip of the probe's entry loop, and a run of 3; a dozen queries of 600, which probe in two full trips of a wave and a tail
    in mode 1.  The hashes are 1 .. 3 000, so a run's entries are its hashes in ascending order.  (The seed: some query holds the first
    and the last entry of every database run, so an entry lost at either end of a run changes a row.)"""
    rng = np.random.default_rng(seed)
    out = []
    for size in BLOCK_RUN_LENGTHS + (BLOCK_QUERY_LENGTH,) * 12:
        hashes = rng.choice(universe, size=size, replace=False)
        out.append({int(h) + 1: int(a) for h, a in zip(hashes, _heavy(rng, size))})
    return out[:len(BLOCK_RUN_LENGTHS)], out[len(BLOCK_RUN_LENGTHS):]


LANE_RUN = 300     # entries of a lane_carry source: lane i of the totals kernel reads entries i and i + 256
LANE_AT = 5


def _run_of(abunds, first=1000):
    """a source whose entry j (hash first + j) has abundance abunds[j]"""
    return {first + j: int(a) for j, a in enumerate(abunds)}


def lane_carry_case(accepted):
    """A source of 300 entries whose two largest abundances sit at entries 5 and 261, which one lane of the totals kernel reads.
    accepted False: both are 2^32 - 1 and the others 1, Σ a² = 2^65 - 2^34 + 300: the lane's own sum wraps, and what it then adds
    to the workgroup's sum does not.  accepted True: 2^32 - 1 and 92 681 there, 408 at entry 0 and 297 small ones (a 3, twenty 2s,
    ones): Σ a² = 2^64 - 1, LIMIT_ABUNDS with 19² + 2² = 365 spread over the padding.  -> (the source, a flat one sharing a hash)"""
    abunds = [1] * LANE_RUN
    if accepted:
        abunds[0] = LIMIT_ABUNDS[2]
        abunds[1] = 3
        abunds[10:30] = [2] * 20
    abunds[LANE_AT] = TOP32
    abunds[LANE_AT + 256] = LIMIT_ABUNDS[1] if accepted else TOP32
    return _run_of(abunds), {1000 + LANE_AT: 1, 7: 1}


def lane_carry_many():
    """-> (db, q): database sources 1 and 3 and query sources 0 and 2 carry; the others are accepted twins or small"""
    bad, small = lane_carry_case(False)
    good, _ = lane_carry_case(True)
    return [good, bad, small, dict(bad)], [dict(bad), good, dict(bad), small]


MASS_N = 16384


def mass_width_case():
    """One pair of sources sharing 16 384 hashes, abundances 2^21 + (j mod 7) in the first and 2^20 + (j mod 5) in the second, and a
    few private hashes each: mass_1 is about 2^35, mass_2 about 2^34, dot about 2^55 and the Σ a² 2^56 and 2^54.
    -> (first, second)"""
    first = {5000 + 3 * j: 2**21 + j % 7 for j in range(MASS_N)}
    second = {5000 + 3 * j: 2**20 + j % 5 for j in range(MASS_N)}
    first.update({5001 + 3 * j: 9 for j in range(10)})
    second.update({5002 + 3 * j: 11 for j in range(10)})
    return first, second


SEAM_RUN = 300


def check_seams_base():
    """Four database sources and four queries of 300 entries, keys ten apart.  Database source 0 ends in 2 990, the key source 1
    begins with, and every other source ends in a key above the first of the next: both are legal, the runs ascend inside a source
    only."""
    def run(first, step, c):
        return {first + step * j: (7 * j + c) % 11 + 1 for j in range(SEAM_RUN)}
    db = [run(0, 10, 0), run(2990, 10, 1), run(2, 10, 2), run(5, 10, 3)]
    q = [run(2, 10, 4), run(0, 10, 5), run(5, 10, 6), run(0, 20, 7)]
    return db, q


def check_seams_variants():
    """name -> ((keys, abund, offsets) of the database, the same of the queries, the message of the refusal).  The first four differ
    from the base in one element: entry 256 of a run is what lane 0 of the check reads on its second trip, and it compares with entry
    255, which lane 255 read on its first."""
    db, q = check_seams_base()
    out = {}

    def variant(name, message, changes):
        sides = {"database": list(arrays(db)), "query": list(arrays(q))}
        for side, source, entry, what, value in changes:
            keys, abund, off = sides[side]
            at = int(off[source]) + entry
            if what == "key":
                keys[at] = value if value is not None else keys[at - 1]
            elif what == "below":
                keys[at] = int(keys[at - 1]) - 1
            else:
                abund[at] = 0
        out[name] = (tuple(sides["database"]), tuple(sides["query"]), message)

    last = SEAM_RUN - 1
    variant("equal_at_255_256", "the run of query source 1 is not strictly ascending", [("query", 1, 256, "key", None)])
    variant("descending_at_255_256", "the run of database source 1 is not strictly ascending", [("database", 1, 256, "below", None)])
    variant("zero_at_256", "query source 2 has an abundance of 0", [("query", 2, 256, "zero", None)])
    variant("zero_at_the_last_entry", "database source 3 has an abundance of 0", [("database", 3, last, "zero", None)])
    three = [("database", 2, 256, "key", None), ("query", 0, 100, "below", None), ("query", 3, 256, "below", None)]
    variant("bad_runs_on_both_sides", "the run of database source 2 is not strictly ascending", three)
    variant("bad_runs_in_the_queries", "the run of query source 0 is not strictly ascending", three[1:])
    variant("zeros_on_both_sides", "database source 1 has an abundance of 0", [("database", 1, 256, "zero", None), ("database", 3, 0, "zero", None), ("query", 0, last, "zero", None)])
    variant("order_fault_behind_a_zero", "the run of query source 3 is not strictly ascending", [("database", 0, 256, "zero", None), ("query", 3, 256, "key", None)])
    return out


def empties_case(seed=3):
    """Database [{}, A, {}] and queries [B, C, {}, {}, D, {}]: an empty source at each end of the database, an empty query between
    full ones, an empty last query, and with a tile of 2 a middle tile without an entry"""
    rng = np.random.default_rng(seed)
    a, b, c, d = ({int(h) + 1: int(x) for h, x in zip(rng.choice(60, size=n, replace=False), _heavy(rng, n))} for n in (40, 30, 20, 25))
    return [{}, a, {}], [b, c, {}, {}, d, {}]


FULL_TILE_QUERIES = 513


def full_tile_case(n=FULL_TILE_QUERIES):
    """513 queries that hold hash 77 with abundances 1 .. 513 and one private hash each: tile 0 is full, query 0 touches tags
    1 .. 511 of it, and tile 1 holds one query, which every query of tile 0 touches"""
    return [], [{77: i + 1, 10**6 + i: 1} for i in range(n)]


TOP64 = 2**64 - 1


def extreme_keys_cases():
    """name -> (db, q).  ends: hashes 0 and 2^64 - 1 with abundances above 1 on both sides, among ordinary hashes and in sources that
    hold one, both or neither.  one_bucket: the queries' keys are 2^63 + i for the even i below 128 (64 of them, one directory
    bucket); the database probes with keys of the bucket that are present, absent between them and absent above the largest, and
    with keys of other buckets.  only_zero: the only query hash is 0, so the table's largest key has no significant bit."""
    base = 2**63
    ends = ([{0: 5, 900: 2, TOP64: 7}, {0: 3}, {TOP64: 4, 12: 1}, {12: 6, 900: 9}],
            [{0: 2, 12: 3, 900: 5, TOP64: 11}, {TOP64: 13}, {0: 17, 900: 4}, {1: 8, TOP64 - 1: 8}, {0: 6, TOP64: 6}])
    one_bucket = ([{base + 1: 4, base + 3: 5, base + 77: 6}, {base + 16: 7, base + 18: 2, base + 5: 9, base + 2**40: 3},
                   {base - 1: 2, 5: 8, base + 126: 10, base + 127: 12}, {base + 2 * i: i + 2 for i in range(64)}],
                  [{base + 16 * j + 2 * i: 8 * i + j + 2 for j in range(8)} for i in range(8)])
    only_zero = ([{0: 5, 9: 2}, {7: 1}, {0: 9}], [{0: 3}, {0: 4}])
    return {"ends": ends, "one_bucket": one_bucket, "only_zero": only_zero}


def nearly_parallel_pairs(seed=17, n=6, size=200):
    """pairs (a, b): a 200-hash sample and the same sample with one abundance one higher, at three scales of abundance (heavy-tailed
    small ones, times 2^8, times 2^16): the cosine is 1 - about 1 / (2 Σ a²)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        scale = (1, 2**8, 2**16)[i % 3]
        a = {int(h) + 1: int(x) * scale + int(rng.integers(0, scale)) for h, x in zip(rng.choice(10**6, size=size, replace=False), _heavy(rng, size))}
        b = dict(a)
        b[sorted(b)[int(rng.integers(0, size))]] += 1
        out.append((a, b))
    return out


def nearly_orthogonal_pairs(seed=19, n=6, size=200):
    """pairs of 200-hash samples that share one hash, held at abundance 1 by both, with the scales of nearly_parallel_pairs
    elsewhere: the cosine is 1 / sqrt(Σ a² Σ b²)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        scale = (1, 2**8, 2**16)[i % 3]
        hashes = rng.choice(10**6, size=2 * size, replace=False) + 1
        a = {int(h): int(x) * scale for h, x in zip(hashes[:size], _heavy(rng, size))}
        b = {int(h): int(x) * scale for h, x in zip(hashes[size:], _heavy(rng, size))}
        a[0] = b[0] = 1
        out.append((a, b))
    return out


def expected_overflows(rows, n_db, tile, capacity):
    """(probe source, query tile) pairs with more than `capacity` rows: a probe source touches exactly the queries of a tile that
    it has a row with, and an emission with more touches than the list holds scans all counters"""
    touched = {}
    for r in rows:
        at = (r[0], (r[1] - n_db) // tile)
        touched[at] = touched.get(at, 0) + 1
    return sum(t > capacity for t in touched.values())

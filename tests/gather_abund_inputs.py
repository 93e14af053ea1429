"""Inputs of the weighted gather tests (tests/test_gather_abund_gpu.py, tests/test_gather_abund_paths_gpu.py).  A case is
(db_runs, q_runs, q_abunds, min_hashes, max_matches); what it is expected to give is gather_abund_restate.gather, and for the hand-made cases also the rows written out
by hand in tests/test_gather_abund_inputs_cpu.py, which shows as well that every builder makes the case it is named for.
Nothing here calls the code under test."""
import numpy as np

TOP32 = 2**32 - 1
#: the sizes of the taken sets: one value, the two of an even median, the edges of ranking in registers (64) and of
#: KSP_GATHER_LONG_SEG (1 024: the candidate is counted by a workgroup)
TAKEN_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025)
#: (lower, upper) middle values on both sides of every digit boundary of a select by 8-bit digits
DIGIT_EDGES = ((255, 256), (65535, 65536), (2**24 - 1, 2**24), (2**32 - 2, TOP32))


def hand_made_cases():
    """name -> (db_runs, q_runs, q_abunds, min_hashes, max_matches)"""
    return {
        # source 0 takes {1, 2, 3} (abundances 5, 1, 9), source 1 then {4, 5} (2, 8): an odd and an even median
        "two_rounds": ([[1, 2, 3], [4, 5]], [[1, 2, 3, 4, 5, 6]], [[5, 1, 9, 2, 8, 100]], 1, 0),
        # source 0 = {1 .. 4}; source 1 = {3, 4, 5, 6} keeps {5, 6} in round 2: its statistics are over 5 and 6 alone, although
        # 3 and 4, which it also holds, are the heavy ones
        "partly_dead_segment": ([[1, 2, 3, 4], [3, 4, 5, 6]], [[1, 2, 3, 4, 5, 6, 7]], [[1, 1, 1000, 1000, 4, 6, 50]], 1, 0),
        # the same two hashes in two queries of one tile, other abundances in each
        "same_hash_two_queries": ([[10, 20]], [[10, 20], [10, 20]], [[3, 5], [70, 0]], 1, 0),
        # a 0 counts as 0; the median of (0, 0, 4) is 0
        "zeros": ([[1, 2, 3]], [[1, 2, 3]], [[0, 4, 0]], 1, 0),
        # two values of 2^32 - 1: the sum of squares needs its upper word
        "upper_word": ([[1, 2]], [[1, 2, 3]], [[TOP32, TOP32, 1]], 1, 0),
        # max_matches cuts the rows; w_found is over the rows reported
        "max_matches_1": ([[1, 2, 3], [4, 5]], [[1, 2, 3, 4, 5]], [[1, 2, 3, 4, 5]], 1, 1),
    }


def _blocks(sizes, first=1000, step=10000):
    return [list(range(first + i * step, first + i * step + n)) for i, n in enumerate(sizes)]


def sizes_case(seed=5):
    """One query of disjoint blocks of TAKEN_SIZES hashes, a source per block: round by round the sources are taken whole, the
    largest first.  The abundances of a block are a permutation of 3, 6, ..., 3n: all different, so an even median is the mean of
    two different values."""
    rng = np.random.default_rng(seed)
    blocks = _blocks(TAKEN_SIZES)
    abund = [int(v) for b in blocks for v in 3 * (rng.permutation(len(b)) + 1)]
    return blocks, [[k for b in blocks for k in b]], [abund], 1, 0


def digit_case(n_side, seed=6):
    """One block per pair of DIGIT_EDGES, of 2 * n_side + 2 hashes: n_side values below the lower middle value (or equal to it),
    the pair, n_side values at or above the upper one — so the two middle values are the pair.  Block sizes differ by 2 so that
    the order of the rounds is fixed; n_side = 1: ranked in registers; n_side = 40: the radix select."""
    rng = np.random.default_rng(seed)
    blocks, abund = [], []
    for i, (lo, hi) in enumerate(DIGIT_EDGES):
        side = n_side + i
        below = [int(v) for v in rng.integers(0, lo + 1, size=side)]
        above = [int(v) for v in rng.integers(hi, min(TOP32, 2 * hi) + 1, size=side)]
        vals = below + [lo, hi] + above
        order = rng.permutation(len(vals))
        abund += [vals[j] for j in order]
        blocks.append(list(range(10**6 * (i + 1), 10**6 * (i + 1) + len(vals))))
    return blocks, [[k for b in blocks for k in b]], [abund], 1, 0


def equal_case():
    """Blocks of 100, 10 and 3 hashes whose abundances are all 7, all 2^32 - 1 and all 0"""
    blocks = _blocks((100, 10, 3))
    return blocks, [[k for b in blocks for k in b]], [[7] * 100 + [TOP32] * 10 + [0] * 3], 1, 0


def dead_part_case(seed=7):
    """Source 0 holds a block of 200 and is taken first; source 1 holds 40 of those (abundances near 2^31) and 50 of its own
    (abundances 1 .. 50): its statistics are over its own 50 alone.  Source 2 the same with 80 + 70, above the threshold of the
    radix select: it is taken second with unique = 70, source 1 third with unique = 50."""
    rng = np.random.default_rng(seed)
    a, own1, own2 = list(range(1000, 1200)), list(range(5000, 5050)), list(range(7000, 7070))
    db = [a, a[:40] + own1, a[10:90] + own2]
    abund = [int(v) for v in rng.integers(2**31, 2**31 + 1000, size=200)] + [int(v) for v in rng.permutation(50) + 1] + [int(v) for v in 5 * rng.permutation(70)]
    return db, [a + own1 + own2], [abund], 1, 0


def tiles_case(n_q=9, seed=8):
    """n_q queries and 12 sources of 30 hashes from 200 values, min_hashes 2: every query has several matches that hide each
    other, and the queries share hashes — with abundances of their own (0 .. 2^20, a few 0)."""
    rng = np.random.default_rng(seed)
    draw = lambda n: [np.sort(rng.choice(200, size=30, replace=False)) for _ in range(n)]   # noqa: E731
    q = draw(n_q)
    abund = [[0 if rng.integers(8) == 0 else int(rng.integers(0, 2**20)) for _ in run] for run in q]
    return draw(12), q, abund, 2, 0


def ones(case):
    """the case with every abundance 1"""
    db, q, _, m, k = case
    return db, q, [[1] * len(run) for run in q], m, k


# ---------------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gather_abund_paths_gpu.py: the states of the select, the carries and the compaction that the cases
# above never reach.  tests/test_gather_abund_inputs_cpu.py shows, from the sorted values alone, that each makes its state.

#: taken sets of the zoo: the smallest radix sizes, the edge of a trip of 4 chunks of 64 (256) and several trips
ZOO_SIZES = (65, 66, 128, 129, 256, 257, 300, 1025)
CARRY_SIZES = (65, 128, 129, 1025)
#: the smallest value whose square is at least 2^63: any two such squares wrap 2^64
WRAP_MIN = 3037000500
#: the 16 values whose bytes are all 0x00 or 0xFF, ascending
CORNERS = tuple(sorted(sum((0xFF if (m >> p) & 1 else 0) << (8 * p) for p in range(4)) for m in range(16)))
DEAD_L = (257, 512, 513, 1024, 1025, 2049)
DEAD_N = (1, 2, 63, 64, 65, 255, 256, 257)


def select_state(values):
    """(branch, r, eq) of the radix select's end over these values, from the sorted values alone: v1 = the lower middle value, eq
    = how many copies of it there are, r = how many of them lie before rank k1; the upper middle value is v1 itself when there is
    one middle rank ("odd") or when more copies follow ("again"), else the smallest value above it ("above")."""
    s = sorted(values)
    k1, k2 = (len(s) - 1) // 2, len(s) // 2
    eq, r = s.count(s[k1]), k1 - s.index(s[k1])
    return ("odd" if k1 == k2 else "again" if r + 1 < eq else "above"), r, eq


def _branch(n, r, eq):
    return "odd" if n % 2 else "again" if r + 1 < eq else "above"


def _fill(rng, count, pool):
    """count values of a pool: a list to choose from, or an inclusive range (lo, hi)"""
    if count == 0:
        return []
    if isinstance(pool, tuple):
        return [int(v) for v in rng.integers(pool[0], pool[1] + 1, size=count, dtype=np.uint64)]
    return [int(pool[i]) for i in rng.integers(0, len(pool), size=count)]


def _place(rng, n, v, r, eq, lo, hi, below=(), above=()):
    """n values, shuffled, whose lower middle value is v with r of its eq copies before rank k1: `below` and `above` are in, the
    rest is drawn from the pools lo (all under v) and hi (all over v)"""
    k1 = (n - 1) // 2
    n_below, n_above = k1 - r, n - (k1 - r) - eq
    assert 0 <= r < eq and n_below >= len(below) and n_above >= len(above), (n, v, r, eq)
    vals = list(below) + _fill(rng, n_below - len(below), lo) + [v] * eq + list(above) + _fill(rng, n_above - len(above), hi)
    assert len(vals) == n and all(0 <= x <= TOP32 for x in vals)
    return [vals[i] for i in rng.permutation(n)]


def _lane_bins(rng, n, byte, r, eq):
    """The lower middle value has `byte` in every position; on every pass the three other bins of the histogram lane that holds
    this digit are filled too (1, 2 and 3 values, under the digits chosen so far): the bins before the chosen one are what the
    lane subtracts from the rank, the chosen one's count is what it hands on."""
    v = byte * 0x01010101
    below, above = [], []
    for p in range(4):
        shift = 24 - 8 * p
        head = v >> (shift + 8) << (shift + 8)
        for i, d in enumerate(x for x in range(byte & ~3, (byte & ~3) + 4) if x != byte):
            for _ in range(i + 1):
                x = head | (d << shift) | int(rng.integers(0, 1 << shift))
                (below if x < v else above).append(x)
    return _place(rng, n, v, r, eq, (0, v - 1), (v + 1, TOP32), below, above)


def _steps(n, shift, base):
    """base + (j // rep << shift): runs of rep equal values that differ in one byte alone — (values, r, eq) by arithmetic"""
    rep = n // 200 + 2
    k1 = (n - 1) // 2
    return [base + ((j // rep) << shift) for j in range(n)], k1 % rep, min(rep, n - k1 // rep * rep)


def ties_named(seed=11):
    """name -> (values, (branch, r, eq)): the multisets of the zoo that are built for a state, at every size of ZOO_SIZES"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in ZOO_SIZES:
        k1 = (n - 1) // 2

        def add(name, values, r, eq):
            out[f"{name}_{n}"] = (values, (_branch(n, r, eq), r, eq))
        v = 0x4D3C2B1A
        # both middle ranks inside a run of 6, other values on both sides
        add("inside", _place(rng, n, v, 2, 6, (0, v - 1), (v + 1, TOP32)), 2, 6)
        # the run of 3 ends at k1; the next value differs in the lowest byte, in the top byte, or is 2^32 - 1
        add("last_low_byte", _place(rng, n, v, 2, 3, (0, v - 1), (v + 1, TOP32), above=[v + 1]), 2, 3)
        add("last_top_byte", _place(rng, n, v, 2, 3, (0, v - 1), (v + (1 << 24), TOP32), above=[v + (1 << 24)]), 2, 3)
        add("last_then_top32", _place(rng, n, v, 2, 3, (0, v - 1), [TOP32]), 2, 3)
        # k1 is a single value, k2 the first copy of a run of 3
        add("first_copy", _place(rng, n, v, 0, 1, (0, v - 1), (v + 7, TOP32), above=[v + 7] * 3), 0, 1)
        # zeros up to k1, then 1; then 2^32 - 1
        add("zeros_then_1", _place(rng, n, 0, k1, k1 + 1, None, (1, TOP32), above=[1]), k1, k1 + 1)
        add("zeros_then_top32", _place(rng, n, 0, k1, k1 + 1, None, [TOP32]), k1, k1 + 1)
        # one bin on three passes: the top three bytes shared; the low three bytes shared
        for name, shift, base in (("low_byte_only", 0, 0xA1B2C300), ("top_byte_only", 24, 0x00345678)):
            values, r, eq = _steps(n, shift, base)
            add(name, [values[i] for i in rng.permutation(n)], r, eq)
        # bytes of 0x00 and 0xFF: lane 0's bin 0 and lane 63's bin 3, in every position
        for v in (0, 0x00FF00FF, 0xFF00FF00, TOP32):
            i = CORNERS.index(v)
            r, eq = (k1, k1 + 6) if v == 0 else (3, n - (k1 - 3)) if v == TOP32 else (3, 9)      # (nothing under 0, nothing over 2^32 - 1)
            add(f"corner_{v:08x}", _place(rng, n, v, r, eq, list(CORNERS[:i]), list(CORNERS[i + 1:])), r, eq)
        # bins 0, 1, 2 and 3 of a lane chosen on every pass, the lane's other bins filled
        for byte, r, eq in ((0x04, 1, 3), (0x45, 1, 2), (0x9E, 2, 3), (0xFB, 1, 2)):
            add(f"lane_bin_{byte & 3}", _lane_bins(rng, n, byte, r, eq), r, eq)
    return out


def ties_random(count=96, seed=12):
    """[(values, the alphabet, (letters, scale, place))]: seeded multisets over alphabets of 2, 3 and 5 values, each alphabet scaled by 1, 2^8, 2^16 and 2^24
    and placed at 0, 255, 2^24 - 1 and just below 2^32; two of three are plain draws, in the third the draw is cut so that a run
    ends at rank k1"""
    rng = np.random.default_rng(seed)
    out = []
    combos = [(m, scale, where) for m in (2, 3, 5) for scale in (1, 1 << 8, 1 << 16, 1 << 24) for where in range(4)]
    for i in range(count):
        m, scale, where = combos[i % len(combos)]
        n = int(ZOO_SIZES[int(rng.integers(len(ZOO_SIZES) - 1))])          # (1 025 is in the named part)
        steps = np.sort(rng.choice(min(200, (TOP32 - 255) // scale), size=m, replace=False))
        steps = steps - steps[0]                                           # the smallest letter is the base itself
        span = int(steps[-1]) * scale
        base = (0, 255, 2**24 - 1, TOP32 - span)[where]
        assert base + span <= TOP32
        alphabet = [base + int(s) * scale for s in steps]
        vals = sorted(alphabet[j] for j in rng.integers(0, m, size=n))
        if i % 3 == 2:   # a run ends at k1: everything behind it is one of the larger letters
            k1 = (n - 1) // 2
            j = min(alphabet.index(vals[k1]), m - 2)
            vals = [min(x, alphabet[j]) for x in vals[:k1 + 1]] + [max(x, alphabet[j + 1]) for x in vals[k1 + 1:]]
        out.append(([vals[j] for j in rng.permutation(n)], alphabet, (m, scale, where)))
    return out


def one_take_per_query(multisets):
    """One query and one source per multiset: the source holds the whole query and nothing else does, so the one row of query i
    takes multiset i (in the order the fill left it).  All in one call."""
    db = [list(range(10**6 * (i + 1), 10**6 * (i + 1) + len(vals))) for i, vals in enumerate(multisets)]
    return db, [list(b) for b in db], [list(vals) for vals in multisets], 1, 0


def zoo_case():
    """(names, case): ties_named and ties_random as one call of one tile"""
    named = ties_named()
    names = list(named) + [f"random_{i}" for i in range(len(ties_random()))]
    return names, one_take_per_query([v for v, _ in named.values()] + [v for v, _, _ in ties_random()])


def carry_sets(seed=13):
    """name -> values: all 2^32 - 1; distinct values whose squares are 2^63 or more, so that any two of a lane wrap its low word,
    whatever slot they came from; those half and half with values below 2^16"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in CARRY_SIZES:
        big = set()
        while len(big) < n:
            big.add(int(rng.integers(WRAP_MIN, 2**32)))
        big = list(big)
        out[f"top32_{n}"] = [TOP32] * n
        out[f"distinct_{n}"] = [big[i] for i in rng.permutation(n)]
        mixed = big[:(n + 1) // 2] + [int(v) for v in rng.integers(0, 2**16, size=n // 2)]
        out[f"mixed_{n}"] = [mixed[i] for i in rng.permutation(n)]
    return out


def carry_case():
    return one_take_per_query(list(carry_sets().values()))


def dead_pairs():
    """(L, n): a block of L slots of which n are alive when it is taken"""
    return [(L, n) for L in DEAD_L for n in sorted(set(DEAD_N + (L - 1,))) if n < L]


def dead_case(pairs=None, alphabet=None, seed=14):
    """Per pair (L, n) one query and two sources.  Source 2q + 1 is a block B of L hashes; source 2q, the killer, holds a random
    L - n of them (K) and n + 1 hashes P of its own: L + 1 hashes, so it wins round 1, and the block is taken in round 2 with
    overlap L and unique n — L - n dead slots spread over its segment, the survivors compacted over trips of 256 entries.  The
    abundances: near 2^31 on K (a dead slot that leaks shows in every statistic), a permutation of 3, 6, ..., 3n on B \\ K — or,
    with `alphabet`, draws from its values: ties among the survivors —, 1 on P."""
    rng = np.random.default_rng(seed)
    db, q, a = [], [], []
    for i, (L, n) in enumerate(dead_pairs() if pairs is None else pairs):
        first = 10**7 * (i + 1)
        B, P = list(range(first, first + L)), list(range(first + 10**6, first + 10**6 + n + 1))
        dead = np.zeros(L, dtype=bool)
        dead[rng.choice(L, size=L - n, replace=False)] = True
        survivors = [int(v) for v in 3 * (rng.permutation(n) + 1)] if alphabet is None else _fill(rng, n, list(alphabet))
        it = iter(survivors)
        ab = [int(rng.integers(2**31, 2**31 + 1000)) if dead[j] else next(it) for j in range(L)]
        db += [[B[j] for j in range(L) if dead[j]] + P, B]
        q.append(B + P)
        a.append(ab + [1] * len(P))
    return db, q, a, 1, 0


#: the pairs that are run again with ties among the survivors, and the three values they are drawn from
DEAD_TIES_PAIRS = ((257, 65), (513, 256), (1025, 257), (1025, 1024))
DEAD_TIES_ALPHABET = (5, 0x01000005, TOP32)


def dead_ties_case():
    return dead_case(DEAD_TIES_PAIRS, DEAD_TIES_ALPHABET, seed=15)


def with_abunds(case, seed=16):
    """A gather_inputs case (db_runs, q_runs, min_hashes, max_matches) with seeded abundances: each 0, 1, a value below 2^20 or one
    of the last four below 2^32, drawn per (query, hash) — a hash gets other values in other queries."""
    rng = np.random.default_rng(seed)
    db, q, m, k = case

    def draw():
        kind = int(rng.integers(4))
        return (0, 1, int(rng.integers(2, 2**20)), TOP32 - int(rng.integers(4)))[kind]
    return db, q, [[draw() for _ in run] for run in q], m, k


def arrays(db_runs, q_runs, q_abunds):
    """(db_keys, db_offsets, q_keys, q_abund, q_offsets) as the ABI takes them"""
    def flat(runs, dtype):
        off = np.zeros(len(runs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in runs])
        vals = np.array([int(v) for r in runs for v in r], dtype=dtype) if int(off[-1]) else np.zeros(0, dtype=dtype)
        return vals, off
    dk, do = flat(db_runs, np.uint64)
    qk, qo = flat(q_runs, np.uint64)
    qa, _ = flat(q_abunds, np.uint32)
    return dk, do, qk, qa, qo

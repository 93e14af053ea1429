"""Inputs of the weighted gather tests (tests/test_gather_abund_gpu.py).  A case is (db_runs, q_runs, q_abunds, min_hashes,
max_matches); what it is expected to give is gather_abund_restate.gather, and for the hand-made cases also the rows written out
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

"""Inputs of the gather tests (tests/test_gather_gpu.py).  A case is (db_runs, q_runs, min_hashes, max_matches); what it is expected
to give is gather_restate.gather, and for the hand-made cases also the rows written out by hand in
tests/test_gather_inputs_cpu.py, which shows as well that every builder makes the case it is named for.  Nothing here calls
the code under test."""
import numpy as np

import query_inputs
from kspider_amd import synth

TOP = 2**64 - 1


def hand_made_cases():
    """name -> (db_runs, q_runs, min_hashes, max_matches)"""
    return {
        # sources 1 and 2 both cover 3 hashes in round 1: the smaller id wins, although source 0 comes first in memory
        "tie_in_round_1": ([[7], [1, 2, 3], [4, 5, 6]], [[1, 2, 3, 4, 5, 6, 7]], 1, 0),
        # 5 / 4 / 3 in round 1; source 0 takes hash 5 away from source 1: 3 / 3 in round 2
        "tie_in_round_2": ([[1, 2, 3, 4, 5], [5, 20, 21, 22], [30, 31, 32]], [[1, 2, 3, 4, 5, 20, 21, 22, 30, 31, 32]], 1, 0),
        "subset_is_never_reported": ([[1, 2], [1, 2, 3, 4], [9]], [[1, 2, 3, 4, 9]], 1, 0),
        "identical_sources": ([[1, 2, 3], [1, 2, 3]], [[1, 2, 3, 4]], 1, 0),
        # source 1 starts with overlap 3 >= 2; source 0 leaves it one hash
        "falls_below_before_it_wins": ([[1, 2, 3, 4], [3, 4, 5]], [[1, 2, 3, 4, 5, 6]], 2, 0),
        # after source 0: source 1 keeps 2 = min_hashes - 1 (not reported), source 2 keeps 3 = min_hashes (reported)
        "threshold_minus_1_and_exact": ([[1, 2, 3, 4, 5], [4, 5, 10, 11], [5, 20, 21, 22]], [[1, 2, 3, 4, 5, 10, 11, 20, 21, 22]], 3, 0),
        # an empty source, an empty query, a query without a match, the keys 0 and 2^64 - 1
        "empties_and_extreme_keys": ([[], [0, TOP], [0], [5]], [[], [0, 7, TOP], [100, 200], [TOP]], 1, 0),
        "max_matches_1": ([[1, 2, 3], [4, 5], [6]], [[1, 2, 3, 4, 5, 6]], 1, 1),
        "max_matches_2": ([[1, 2, 3], [4, 5], [6]], [[1, 2, 3, 4, 5, 6]], 1, 2),
    }


def shared_words_case(n_q=40):
    """One key (42) held by all of n_q two-hash queries: its holder slots are neighbours, so alive bits of different queries sit in
    one word.  Source 0 = {42} and source 1 = every query's own hash tie at 1 in round 1 for every query: all queries take source
    0 in round 1 and source 1 in round 2."""
    return [[42], [1000 + i for i in range(n_q)]], [[42, 1000 + i] for i in range(n_q)], 1, 0


def chain_blocks(n, first=10**6):
    """n disjoint blocks of n + 2, n + 1, ..., 3 hashes: strictly decreasing, the last contributes 3"""
    blocks, at = [], first
    for i in range(n):
        blocks.append(list(range(at, at + n + 2 - i)))
        at += n + 2 - i
    return blocks


def chain_case(n=70, max_matches=0):
    """n sources, each a core of 5 hashes that all share plus a block of its own; the blocks shrink strictly (n + 2 .. 3 hashes),
    so source i wins round i + 1 with unique = its block (the first also takes the core) and overlap = block + 5.  min_hashes =
    3: the last source still passes.  n + 1 rounds without max_matches."""
    core = [1, 2, 3, 4, 5]
    blocks = chain_blocks(n)
    return [core + b for b in blocks], [core + [k for b in blocks for k in b]], 3, max_matches


def finish_case():
    """Three queries of one tile that finish after 0, 1 and 40 rows: no match, one match, a chain of 40."""
    db, q, m, _ = chain_case(40)
    return db + [[7, 8, 9]], [[50, 51, 52], [7, 8, 9, 10], q[0]], m, 0


SEGMENT_LENGTHS = (63, 64, 65, 255, 256, 257)


def segment_case():
    """Candidates whose segments are 63 / 64 / 65 and 255 / 256 / 257 slots: source i holds a block of its own of that many hashes
    less 2, and 2 hashes of the next source's block, all in the one query; one more source holds 3 hashes of every block (18 in all:
    the others cover them first, it is never reported)."""
    at, blocks = 1000, []
    for n in SEGMENT_LENGTHS:
        blocks.append(list(range(at, at + n - 2)))
        at += 1000
    db = [blocks[i] + blocks[(i + 1) % len(blocks)][:2] for i in range(len(blocks))]
    db.append([k for b in blocks for k in b[5:8]])
    return db, [[k for b in blocks for k in b] + [5, 6]], 1, 0


def tiles_case(n_q, seed=3):
    """n_q queries and 30 database sources of 40 hashes from 300 values: every query has several matches that hide each other."""
    rng = np.random.default_rng(seed + n_q)
    draw = lambda n: [np.sort(rng.choice(300, size=40, replace=False)) for _ in range(n)]   # noqa: E731
    return draw(30), draw(n_q), 2, 0


def random_case():
    """query_inputs.random_case(): 260 + 40 sources of a clustered set"""
    db, q = query_inputs.random_case()
    return db, q, 3, 0


def sample_case(n_db=100, mean_size=5000, n_pick=10, n_noise=2000, seed=9):
    """The shape tools/gather_times.py times, at 1/100 of its size: a clustered database and one query that is the union of
    random halves of n_pick of its sources plus noise."""
    sk = synth.generate("C2", n_sources=n_db, mean_size=mean_size, cluster_cap=10, seed=seed)
    return [sk.run(s) for s in range(sk.n_sources)], [synth.gather_sample(sk, n_pick, n_noise, seed)], 5, 0


def wide_case(n_q=1100, n_db=5):
    """One tile wider than the touched list, the tail's 1 024 threads and (in candidates) the first candidate buffer: n_db sources
    of 1 .. n_db keys of their own plus one key of the next source; every query holds all 15 keys but one (every 7th: but up to
    three) and a key of its own, so every source shares keys with every query and the sources hide each other."""
    core = [[1000 * (s + 1) + i for i in range(s + 1)] for s in range(n_db)]
    allcore = [k for c in core for k in c]
    db = [core[s] + core[(s + 1) % n_db][:1] for s in range(n_db)]
    q = []
    for j in range(n_q):
        drop = {allcore[j % len(allcore)]}
        if j % 7 == 0:
            drop |= {allcore[(j // 7) % len(allcore)], allcore[(j // 7 + 4) % len(allcore)]}
        q.append([k for k in allcore if k not in drop] + [10**6 + j])
    return db, q, 2, 0


def list_edge_case(n_share):
    """n_share queries {77, 78, own key} at min_hashes 2: source 0 is a candidate of every query (both sweeps see it touch n_share
    queries), source 1 touches every query but is only dropped (the counting sweep alone), source 2 touches none."""
    return [[77, 78, 5], [78, 6], [6, 5]], [[77, 78, 10**6 + j] for j in range(n_share)], 2, 0


def seam_case():
    """Under a tile of 2: a tile of empty queries, a tile whose queries share no key with the database, a tile with rows (queries
    4 and 5: tiles_case(5)'s first two), a last tile of one empty query."""
    db, q, m, _ = tiles_case(5)
    return db, [[], [], [1000, 1001, 1002], [2000, 2001], q[0], q[1], []], m, 0


def block_case():
    """query_inputs.block_case(): database runs of 255 / 256 / 257 / 1 023 / 1 024 / 1 025 and 3 entries at min_hashes 2"""
    db, q = query_inputs.block_case()
    return db, q, 2, 0


SWITCH_CHOICES = (("KSP_QUERY_TILE", ("1", "2", "3", None)), ("KSP_QUERY_LIST", ("1", "2", "3", None)), ("KSP_QUERY_LONG_RUN", ("1", "8", None)),
                  ("KSP_GATHER_LONG_SEG", ("1", "4", None)), ("KSP_GATHER_TAIL", ("0", "1")), ("KSP_GATHER_TAIL_CANDS", ("0", "3", None)),
                  ("KSP_GATHER_MAX_WORKGROUPS", ("1", "2", None)))


def switch_cases(n=48, seed=20261020):
    """n small random cases, each with an independent draw of every switch: [(case, {switch: value or None = unset})].  1 .. 12
    sources and 1 .. 9 queries of 0 .. 30 keys from 12, 40 or 90 values, min_hashes of 1 / 2 / 3 / 5, max_matches of 0 / 0 / 1 / 2."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_db, n_q, universe = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.choice([12, 40, 90]))
        draw = lambda k: [np.sort(rng.choice(universe, size=min(int(rng.integers(0, 31)), universe), replace=False)) for _ in range(k)]   # noqa: E731
        case = (draw(n_db), draw(n_q), int(rng.choice([1, 2, 3, 5])), int(rng.choice([0, 0, 1, 2])))
        out.append((case, {name: values[int(rng.integers(len(values)))] for name, values in SWITCH_CHOICES}))
    return out


def slots(db_runs, q_runs, min_hashes):
    """Σ overlap over the candidates: the (source, query) pairs that share min_hashes keys or more"""
    sets = [set(int(k) for k in run) for run in db_runs]
    shared = [len(S & set(int(k) for k in run)) for run in q_runs for S in sets]
    return sum(n for n in shared if n >= min_hashes)


def by_tile(case, tile, restate):
    """What a case gives when its queries are taken `tile` at a time (queries are independent; a tile's first query is added to
    the query index): (rows, {candidates, dropped, fell_below, slots: sums over the tiles; passes: the tiles that have an entry;
    rounds: Σ max(iterations) over the tiles that have a candidate — a tile without one runs no round}).  `restate` is
    gather_restate.gather."""
    db, q, m, k = case
    rows, total = [], {"candidates": 0, "dropped": 0, "fell_below": 0, "slots": 0, "passes": 0, "rounds": 0}
    for q0 in range(0, len(q), tile):
        part, counts = q[q0:q0 + tile], {}
        rows += [(r[0] + q0,) + r[1:] for r in restate(db, part, m, k, counts)]
        for name in ("candidates", "dropped", "fell_below"):
            total[name] += counts[name]
        total["slots"] += slots(db, part, m)
        total["passes"] += any(len(run) for run in part)
        total["rounds"] += max(counts["iterations"]) if counts["candidates"] else 0
    return rows, total


def arrays(db_runs, q_runs):
    """(db_keys, db_offsets, q_keys, q_offsets) as the ABI takes them"""
    sk = query_inputs.concat(db_runs, q_runs)
    return query_inputs.split(sk, len(db_runs))

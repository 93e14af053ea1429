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


def arrays(db_runs, q_runs):
    """(db_keys, db_offsets, q_keys, q_offsets) as the ABI takes them"""
    sk = query_inputs.concat(db_runs, q_runs)
    return query_inputs.split(sk, len(db_runs))

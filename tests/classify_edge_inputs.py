"""Seeded inputs of the second classify suite (tests/test_classify_edge_inputs_cpu.py, tests/test_classify_edges_gpu.py): streams
of several tiles whose kept windows are sparse, a model of the drain schedule of k_classify_hash, and references that shape the
table — keys one beside a probed hash, one crowded bucket of the directory, exact key counts, more references than a query tile,
a designed matrix of hit counts.  Every builder works on the restated hashes (tests/classify_restate.py); nothing here calls the
library.  tests/test_classify_edge_inputs_cpu.py checks that each edge is there."""
import functools
import random

import classify_inputs as CI
import sketch_inputs as I
import sketch_restate as R

FULL = CI.FULL
T = I.TILE

# These mirror kRound and kListCap of kspider_amd/csrc/classify_kernels.hip.h: a round is four trips of a workgroup of 256 over
# the positions of a tile, the list in LDS holds two rounds.
K_ROUND = 1024
K_LIST_CAP = 2048

N_BYTES = 6 * T + 101   # 6 T + 100 bases and the newline: seven tiles


def sparse(k, seed=41):
    """One record of 6 T + 100 bases, 10 % of them in lower case, 40 random positions set to N, and a trailing newline.  (The
    seed is one at which every workgroup of a grid of 3 ends on a list that is not empty at k = 21 and at k = 33:
    tests/test_classify_edge_inputs_cpu.py checks the whole schedule.)"""
    rng = random.Random(seed * 1000 + k)
    s = list(I.bases(rng, 6 * T + 100, lower=0.1))
    for _ in range(40):
        s[rng.randrange(len(s))] = "N"
    seq = ("".join(s) + "\n").encode()
    return I.Case("sparse", seq, [0, len(seq)])


def sparse_records(k, seed=32):
    """The length of sparse(k), cut into records: two contigs of 600 bases, the first over the tile edge at T, the second over the
    one at 5 T, and before, between and behind them reads of 10 to 200 bases (about 300: short ones are more frequent), some
    shorter than k.  Every 25th read is empty: by turns a record of no byte at all and one of a newline alone.  The stream holds
    no break byte but the newline that ends a record, and every 7th read has none: it abuts the next record base to base."""
    rng = random.Random(seed * 1000 + k)
    starts = [T - 300, 5 * T - 300, N_BYTES]   # the contigs' first bytes, and the end
    recs, pos, n_reads = [], 0, 0
    for i, stop in enumerate(starts):
        while pos < stop:
            n_reads += 1
            gap = stop - pos
            if gap <= 201:   # the last read before a contig (or the end) fills the gap
                text = I.bases(rng, gap - 1) + "\n"
            elif n_reads % 25 == 0:
                text = "" if n_reads % 50 == 0 else "\n"
            else:
                text = I.bases(rng, min(rng.randint(10, 200), rng.randint(10, 200), gap - 12), lower=0.1) + ("" if n_reads % 7 == 0 else "\n")
            recs.append(text)
            pos += len(text)
        if i < 2:
            recs.append(I.bases(rng, 600, lower=0.1) + "\n")
            pos += 601
    seq = "".join(recs).encode()
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    assert len(seq) == N_BYTES
    return I.Case("sparse_records", seq, off)


def matrix_records(k, n, seed=33):
    """n reads of k + 8 bases, each followed by a newline: nine windows per record."""
    rng = random.Random(seed * 1000 + k)
    recs = [I.bases(rng, k + 8) + "\n" for _ in range(n)]
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    return I.Case("matrix_records", "".join(recs).encode(), off)


@functools.lru_cache(maxsize=None)
def case_of(name, k):
    return {"sparse": lambda: sparse(k), "sparse_records": lambda: sparse_records(k), "matrix_records": lambda: matrix_records(k, len(MATRIX))}[name]()


@functools.lru_cache(maxsize=None)
def windows_of(name, k):
    """Per record of a case the windows as [(position in the stream, hash)], in order of position."""
    case = case_of(name, k)
    out = []
    for r in range(len(case.offsets) - 1):
        a, b = case.offsets[r], case.offsets[r + 1]
        kmers = R.source_kmers(case.seq[a:b], k)
        out.append([(a + p, h) for (p, _), h in zip(kmers, R.kmer_hashes([text for _, text in kmers]))])
    return out


def kept_of(name, k, max_hash=FULL):
    """What classify_restate.record_hashes gives for a case (the CPU test compares them): per record the kept hashes in order of position."""
    return [[h for _, h in run if h <= max_hash] for run in windows_of(name, k)]


def keep_positions(name, k, max_hash):
    """The stream positions at which a kept window starts, ascending."""
    return sorted(p for run in windows_of(name, k) for p, h in run if h <= max_hash)


def drains(keep_positions, n_bytes, grid):
    """The schedule of k_classify_hash, restated: workgroup w takes the tiles w, w + grid, ...; after every round of K_ROUND
    positions it drains its list if that holds more than K_LIST_CAP - K_ROUND kept window starts, and it drains once more behind
    its last tile.  Per workgroup: (the sizes of the drains inside the loop, the size of the last one)."""
    n_tiles = -(-n_bytes // T)
    per_round = {}
    for p in keep_positions:
        per_round[p // K_ROUND] = per_round.get(p // K_ROUND, 0) + 1
    out = []
    for w in range(min(grid, n_tiles)):
        held, inside = 0, []
        for tile in range(w, n_tiles, grid):
            for r0 in range(tile * T, (tile + 1) * T, K_ROUND):
                held += per_round.get(r0 // K_ROUND, 0)
                assert held <= K_LIST_CAP
                if held > K_LIST_CAP - K_ROUND:
                    inside.append(held)
                    held = 0
        out.append((inside, held))
    return out


def distinct(kept):
    return sorted({h for run in kept for h in run})


def nowhere(kept, n, seed, taken=()):
    """n random hashes that no record holds (and that are not in `taken`), ascending."""
    rng = random.Random(seed)
    everything = {h for run in kept for h in run} | set(taken)
    out = set()
    while len(out) < n:
        h = rng.getrandbits(64)
        if h not in everything:
            out.add(h)
    return sorted(out)


# the references of near_miss()
BESIDE, ENDS, EVERY_2ND, AT_M = range(4)


def near_miss(kept, at=None):
    """[BESIDE: h - 1 and h + 1 for every third distinct record hash h, and no record hash; ENDS: 0 and 2^64 - 1; EVERY_2ND: every
    2nd record hash, the hits beside the misses]; with `at` = m one reference more, AT_M: m and m + 1."""
    everything = distinct(kept)
    have = set(everything)
    assert 0 not in have and FULL not in have
    beside = sorted({x for h in everything[::3] for x in (h - 1, h + 1)} - have)
    refs = [beside, [0, FULL], everything[::2]]
    if at is not None:
        refs.append([at, at + 1])
    return refs


def skew_target(kept):
    everything = distinct(kept)
    return everything[len(everything) // 2]


# the references of skewed()
DECOYS, REAL = range(2)


def skewed(kept, n=5000, seed=34):
    """[DECOYS: n keys that equal the record hash h* = skew_target(kept) in all but the low 16 bits, none of them a record hash;
    REAL: h* and every 5th record hash].  The decoys and h* lie in one bucket of the directory, which so holds n + 1 keys."""
    everything = distinct(kept)
    have = set(everything)
    star = skew_target(kept)
    rng = random.Random(seed)
    lows = rng.sample(range(1 << 16), n + 8)
    decoys = sorted(x for x in ((star & ~0xFFFF) | low for low in lows) if x not in have)[:n]
    assert len(decoys) == n
    return [decoys, sorted(set(everything[::5]) | {star})]


SIZES = [(1, "smallest"), (1, "largest"), (8, None), (9, None), (4096, None), (4097, None)]


def sized(kept, U, which=None, seed=35):
    """References whose union holds exactly U distinct keys.  U = 1: the smallest (or the largest) record hash alone, beside an
    empty reference.  Otherwise U // 2 record hashes, evenly spaced, padded with random hashes that occur nowhere, dealt to three
    references that overlap: the even ranks, the odd ranks, every third rank."""
    everything = distinct(kept)
    if U == 1:
        return [[], [everything[0] if which == "smallest" else everything[-1]]]
    real = everything[::len(everything) // (U // 2)][:U // 2]
    assert len(real) == U // 2
    keys = sorted(real + nowhere(kept, U - len(real), seed * 10000 + U))
    assert len(set(keys)) == U
    return [keys[::2], keys[1::2], keys[::3]]


N_MANY = 2051
MANY_EMPTY = [0, 1] + list(range(1000, 1010)) + [N_MANY - 1]


def many_shared(kept):
    everything = distinct(kept)
    return everything[len(everything) // 3]


def many(kept, n_refs=N_MANY, seed=36):
    """n_refs references, those of MANY_EMPTY empty.  The record hash many_shared(kept) is held by every other reference; every
    other record hash goes to one or to two references, by a seeded draw."""
    assert n_refs == N_MANY
    rng = random.Random(seed)
    holders = [q for q in range(n_refs) if q not in set(MANY_EMPTY)]
    shared = many_shared(kept)
    refs = [[] for _ in range(n_refs)]
    for h in distinct(kept):
        for q in (holders if h == shared else rng.sample(holders, rng.randint(1, 2))):
            refs[q].append(h)
    return [sorted(q) for q in refs]


# the named rows of the shipped matrix, and what the summary says about them: (best_ref, second_hits)
NAMED_ROWS = [[2, 5, 5, 3, 5], [5, 2, 3, 0, 0], [2, 3, 5, 0, 0], [3, 5, 2, 0, 0], [4, 4, 4, 4, 4], [0, 0, 0, 0, 7]]
NAMED_SUMMARY = [(1, 5), (0, 3), (2, 3), (1, 3), (0, 4), (4, 0)]
NAMED_AT = 40    # the record of the first named row
ZEROS_AT = range(100, 140, 2)


def _matrix(n=300, seed=37):
    """300 records (two blocks of the summary kernel) by five references: seeded counts of 0 to 6, the named rows from record
    NAMED_AT on, all-zero rows at the first record, at the last and at every second record of ZEROS_AT."""
    rng = random.Random(seed)
    m = [[rng.randint(0, 6) if rng.random() < 0.6 else 0 for _ in range(5)] for _ in range(n)]
    for i, row in enumerate(NAMED_ROWS):
        m[NAMED_AT + i] = list(row)
    for r in [0, n - 1] + list(ZEROS_AT):
        m[r] = [0] * 5
    return m


MATRIX = _matrix()


def hit_matrix(kept, m):
    """For records whose hash sets are disjoint: reference q holds the first m[r][q] distinct hashes of every record r, so that
    hits(r, q) = m[r][q]."""
    assert len(kept) == len(m)
    firsts = [list(dict.fromkeys(run)) for run in kept]
    assert sum(len(f) for f in firsts) == len({h for f in firsts for h in f}), "the records share a hash"
    refs = []
    for q in range(len(m[0])):
        assert all(m[r][q] <= len(firsts[r]) for r in range(len(m)))
        refs.append(sorted(h for r in range(len(m)) for h in firsts[r][:m[r][q]]))
    return refs


def table_cases(kept):
    """Every table-shape case on records whose kept hashes are given: [(name, references)]."""
    out = [("near_miss", near_miss(kept)), ("skewed", skewed(kept))]
    out += [(f"sized{U}{which or ''}", sized(kept, U, which)) for U, which in SIZES]
    return out


# ---- the session with hostile ids: batches of (segment texts, record ids)
SESSION_PLAN = [[5, 2, 5, 0], [1], [70000, 3], [4]]
# one id per batch, each beyond twice the room the kept-window counters have by then (1, 2, 4, 10, 41: five growths), then one below
GROWTH_PLAN = [[0], [1], [3], [9], [40], [2]]


def session_batches(k, plan=SESSION_PLAN, breaks_only=(4,), seed=38):
    """The batches of a plan as (bytes, segment offsets, record ids); SESSION_PLAN: ids [5, 2, 5, 0] — record 5 in two segments that
    are not adjacent —, then [1], then [70000, 3], then a batch of break bytes alone for record 4.  Also the text of every record
    that has one: its segments joined by a break byte."""
    rng = random.Random(seed * 1000 + k)
    batches, texts = [], {}
    for ids in plan:
        segs = ["NN\n-N\n" if r in breaks_only else I.bases(rng, rng.randint(150, 400), lower=0.1) + "\n" for r in ids]
        off = [0]
        for s in segs:
            off.append(off[-1] + len(s))
        batches.append(("".join(segs).encode(), off, ids))
        for r, s in zip(ids, segs):
            texts[r] = texts[r] + "N" + s if r in texts else s
    return batches, texts


def records_of(texts, n_records):
    """(stream, offsets) of the records 0 .. n_records - 1, a record without a text being empty."""
    off, parts = [0], []
    for r in range(n_records):
        parts.append(texts.get(r, ""))
        off.append(off[-1] + len(parts[-1]))
    return "".join(parts).encode(), off

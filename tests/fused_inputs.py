"""Seeded hostile colour indexes for the fused drop-in calls (tests only, numpy only): what tests/test_fused_inputs_cpu.py
checks with the oracle alone and tests/test_fused_random_gpu.py runs through every kspider_pairwise_* call.

Every shape plants its features first and randomises the rest of the index around them from the seed:

  "mixed"      120 sources with sparse ids below NN = 156 (NN itself is no id), several hundred colours.  The sources are
               split into populations that decide which pairs are real rows (a weighted colour in common) and which exist
               only with shared_kmers = 0 (weight-0 colours in common and no other):
                 core     70 sources of one weighted colour that holds them all, so every core pair is a real row
                 fringe   26 sources of a few small weighted colours: most of their pairs are no real rows
                 z-only    4 sources of weight-0 colours only
                 islands   4 x 3 sources, each island a triangle of real rows and nothing else — but one weight-0 colour
                           joins island 1 to island 2 (both ends count k-mers: an ordinary 0-valued row) and one joins
                           island 3 to island 4 (its source_2 counts 0 k-mers: a NaN row)
                 unsure    3 pairs (a, b): a weighted colour of weight 1, a weight-0 colour, a counts >= 5 000 k-mers, b
                           counts 0 — the real row has min containment <= 1 / 5 000, and the zero pair is a NaN row
                 single    2 sources of single-source colours only
               One weight-0 colour of 40 members (fringe, z-only and 10 of the core), more weight-0 colours that overlap
               it, colours that repeat another's member set with another weight, 30 % of all colours weighing 0, one
               fringe source without a k-mer count entry, 13 sources counting 0 k-mers — among them the smallest and the
               largest fringe id, so that zero-only pairs have the 0 on the source_1 side, the source_2 side and both.
               (One colour cannot hold EVERY source while a source occurs in single-source colours only and while there
               are pairs without a real row: "every source" is every source of the core.)
  "tiny"       7 .. 12 sources with the same ingredients, one of each.
  "all_zero"   30 sources, every colour weighs 0: no posting at all.
  "one_edge"   10 sources, one weighted colour of two sources among weight-0 colours.
  "no_counts"  "tiny" with every source counting 0 k-mers: every value is a NaN or an infinity.

A source that counts k-mers counts at least the sum of its colours' weights: no finite containment is above 1."""
import math
from dataclasses import dataclass, field, replace

import numpy as np

SHAPES = ("mixed", "tiny", "all_zero", "one_edge", "no_counts")
DISTS = {"min_cont": 3, "avg_cont": 4, "max_cont": 5}


@dataclass
class FusedInput:
    shape: str
    seed: int
    color_off: np.ndarray
    sources: np.ndarray
    color_w: np.ndarray
    group_ids: np.ndarray           # the groups with a k-mer count entry ...
    kmer_counts: np.ndarray         # ... and their counts
    NN: int                         # rows of .namesMap
    ids: list = field(default_factory=list)          # every id that occurs in a colour, ascending
    unsure: list = field(default_factory=list)       # the pairs planted for the cut's `unsure` branch
    zero_bridges: list = field(default_factory=list) # the zero-only pairs that alone connect two components of real rows
    rank_flip: tuple = ()           # (smaller id, larger id): tied without the zero-only rows, the larger one first with them
    single_only: list = field(default_factory=list)
    zero_only: list = field(default_factory=list)    # sources of weight-0 colours only
    no_count: list = field(default_factory=list)     # ids without a k-mer count entry


class _Builder:
    def __init__(self, rng, n_sources, NN):
        self.rng = rng
        self.NN = NN
        self.ids = np.sort(rng.choice(np.arange(1, NN), size=n_sources, replace=False)).tolist()   # (NN itself is no id)
        self.free = list(rng.permutation(self.ids))
        self.colours = []               # (members, weight)
        self.zero_count = set()
        self.no_count = set()
        self.big_count = set()

    def take(self, n):
        out, self.free = sorted(int(x) for x in self.free[:n]), self.free[n:]
        assert len(out) == n
        return out

    def colour(self, members, weight):
        members = sorted(set(int(m) for m in members))
        assert members
        self.colours.append((members, int(weight)))

    def random_colours(self, n, pool, lo, hi, zero_share):
        for _ in range(n):
            size = int(self.rng.integers(lo, min(hi, len(pool)) + 1))
            w = 0 if self.rng.random() < zero_share else int(self.rng.integers(1, 41))
            self.colour(self.rng.choice(pool, size=size, replace=False), w)

    def repeats(self, n):
        """n colours that repeat another colour's member set with a different weight (0 becomes > 0 and the other way)."""
        multi = [c for c in self.colours if len(c[0]) >= 2]
        for i in self.rng.choice(len(multi), size=min(n, len(multi)), replace=False):
            members, w = multi[int(i)]
            self.colour(members, 0 if w and self.rng.random() < 0.4 else w + int(self.rng.integers(1, 9)))

    def finish(self, shape, seed, all_counts_zero=False, **meta):
        rng = self.rng
        wsum = {}
        for members, w in self.colours:
            if len(members) >= 2:
                for m in members:
                    wsum[m] = wsum.get(m, 0) + w
        counts = {}
        for g in self.ids:
            if g in self.no_count:
                continue
            if all_counts_zero or g in self.zero_count:
                counts[g] = 0
            else:
                ws = wsum.get(g, 0)
                counts[g] = ws + 1 + int(rng.integers(0, 4 * ws + 50)) + (5000 if g in self.big_count else 0)
        spare = sorted(set(range(1, self.NN)) - set(self.ids))
        if spare:                                   # a group with a count that occurs in no colour: a row of seqToKmersNo only
            counts[spare[int(rng.integers(0, len(spare)))]] = 0 if all_counts_zero else 77
        order = rng.permutation(len(self.colours))
        off, src, w = [0], [], []
        for i in order:
            members, weight = self.colours[int(i)]
            src += [int(m) for m in rng.permutation(members)]
            off.append(len(src))
            w.append(weight)
        gids = [int(g) for g in rng.permutation(sorted(counts))]
        return FusedInput(shape=shape, seed=seed, color_off=np.array(off, dtype=np.uint32), sources=np.array(src, dtype=np.uint32),
                          color_w=np.array(w, dtype=np.uint32), group_ids=np.array(gids, dtype=np.uint32),
                          kmer_counts=np.array([counts[g] for g in gids], dtype=np.uint32), NN=self.NN,
                          ids=sorted({m for members, _ in self.colours for m in members}),   # (a source the random colours missed is a group with a count only)
                          no_count=sorted(self.no_count), **meta)

    def plant_unsure(self, pair):
        """(a, b), a < b: one shared k-mer, b counts 0 k-mers, a counts >= 5 000 — and the pair is a zero pair too."""
        a, b = pair
        self.colour([a, b], 1)
        self.colour([a, b], 0)
        self.big_count.add(a)
        self.zero_count.add(b)
        return (a, b)


def _mixed(seed):
    rng = np.random.default_rng([seed, 1])
    B = _Builder(rng, 120, 156)
    core, fringe, zonly, single = B.take(70), B.take(26), B.take(4), B.take(2)
    islands = [B.take(3) for _ in range(4)]
    unsure = [tuple(B.take(2)) for _ in range(3)]
    assert not B.free
    B.colour(core, 1)                                                   # every core pair is a real row
    B.random_colours(int(rng.integers(260, 420)), core, 2, 5, 0.3)
    B.random_colours(int(rng.integers(110, 200)), core + fringe, 2, 5, 0.3)
    core10 = [int(x) for x in rng.choice(core, size=10, replace=False)]
    B.colour(fringe + zonly + core10, 0)                                # 40 members: 780 zero pairs, 45 of them real rows at least
    B.random_colours(15, fringe + zonly + core10, 2, 5, 1.0)            # weight-0 colours that overlap it
    B.repeats(30)
    for s in single:
        B.colour([s], 0)
        B.colour([s], 5)
    for s in rng.choice(core, size=8, replace=False):
        B.colour([s], int(rng.integers(0, 3)))
    for isl in islands:                                                 # a triangle of real rows with three different weights
        B.colour(isl, int(rng.integers(3, 20)))
        B.colour(isl[:2], int(rng.integers(1, 9)))
    x, y = islands[0][2], islands[1][0]
    B.colour([x, y], 0)                                                 # islands 1 and 2: an ordinary 0-valued row
    bridges = [tuple(sorted((x, y)))]
    p, q = sorted((islands[2][int(rng.integers(0, 3))], islands[3][int(rng.integers(0, 3))]))
    B.colour([p, q], 0)                                                 # islands 3 and 4: a NaN row (source_2 counts 0 k-mers)
    B.zero_count.add(q)
    bridges.append((p, q))
    for pair in unsure:
        B.plant_unsure(pair)
    B.zero_count.update([fringe[0], fringe[-1]])                        # the 0 on the source_1 side, the source_2 side and both
    B.zero_count.update(int(v) for v in rng.choice(fringe[1:-1], size=3, replace=False))
    B.zero_count.update(int(v) for v in rng.choice(zonly, size=2, replace=False))
    B.zero_count.update(int(v) for v in rng.choice(core, size=2, replace=False))
    B.no_count.add(next(f for f in fringe[1:-1] if f not in B.zero_count))
    return B.finish("mixed", seed, unsure=unsure, zero_bridges=bridges, rank_flip=(islands[0][0], islands[0][2]), single_only=single,
                    zero_only=zonly)


def _tiny(seed, all_counts_zero=False):
    rng = np.random.default_rng([seed, 2])
    n = int(rng.integers(7, 13))
    B = _Builder(rng, n, math.ceil(1.3 * n) + 1)
    core, pair, z, single = B.take(3), tuple(B.take(2)), B.take(1), B.take(1)
    rest = B.take(len(B.free))
    B.colour(core, int(rng.integers(2, 10)))
    B.colour(core[:2], int(rng.integers(1, 5)))
    B.colour(core[1:], 0)                                               # a zero pair that is a real row
    B.colour([core[2], z[0]], 0)                                        # zero-only
    B.colour([core[0], z[0]] + rest[:1], 0)
    B.random_colours(3 + len(rest), core + rest, 2, 4, 0.3)
    B.repeats(2)
    B.colour(single, 3)
    B.colour(single, 0)
    B.plant_unsure(pair)
    B.zero_count.add(z[0])
    if rest and rng.random() < 0.5:
        B.zero_count.add(rest[-1])
    if len(rest) >= 2:
        B.no_count.add(rest[0])
    return B.finish("no_counts" if all_counts_zero else "tiny", seed, all_counts_zero=all_counts_zero, unsure=[pair], single_only=single, zero_only=z)


def _all_zero(seed):
    rng = np.random.default_rng([seed, 3])
    B = _Builder(rng, 30, 40)
    pool = B.take(30)
    B.colour(pool[:12], 0)
    B.random_colours(25, pool[:27], 2, 5, 1.0)
    used = {m for members, _ in B.colours for m in members}
    B.colour([pool[0]] + [p for p in pool[:27] if p not in used], 0)    # (whoever the random colours missed)
    for s in pool[27:]:
        B.colour([s], 0)
    B.zero_count.update(int(v) for v in rng.choice(pool[:27], size=4, replace=False))
    B.no_count.add(next(p for p in pool[:27] if p not in B.zero_count))
    return B.finish("all_zero", seed, single_only=pool[27:])


def _one_edge(seed):
    rng = np.random.default_rng([seed, 4])
    B = _Builder(rng, 10, 14)
    pool = B.take(10)
    B.random_colours(8, pool, 2, 4, 1.0)
    pair = [int(v) for v in rng.choice(pool, size=2, replace=False)]
    B.colour(pair, 3)
    B.zero_count.add(next(p for p in pool if p not in pair))
    return B.finish("one_edge", seed)


def make(seed: int, shape: str) -> FusedInput:
    if shape == "mixed":
        return _mixed(seed)
    if shape == "tiny":
        return _tiny(seed)
    if shape == "no_counts":
        return _tiny(seed, all_counts_zero=True)
    if shape == "all_zero":
        return _all_zero(seed)
    if shape == "one_edge":
        return _one_edge(seed)
    raise ValueError(shape)


def with_counts(fi: FusedInput) -> FusedInput:
    """fi with a k-mer count for every source (the ANI calls refuse a NaN row): 0 and missing counts become the sum of the
    source's colour weights + 1 + (id mod 50), so no containment is above 1."""
    wsum = {}
    for c in range(len(fi.color_w)):
        members = fi.sources[fi.color_off[c]:fi.color_off[c + 1]].tolist()
        if len(members) >= 2:
            for m in members:
                wsum[m] = wsum.get(m, 0) + int(fi.color_w[c])
    counts = dict(zip(fi.group_ids.tolist(), fi.kmer_counts.tolist()))
    for g in fi.ids:
        if not counts.get(g, 0):
            counts[g] = wsum.get(g, 0) + 1 + g % 50
    gids = fi.group_ids.tolist() + [g for g in fi.ids if g not in set(fi.group_ids.tolist())]
    return replace(fi, group_ids=np.array(gids, dtype=np.uint32), kmer_counts=np.array([counts[g] for g in gids], dtype=np.uint32),
                   no_count=[], unsure=[])


def write(oracle_lib, prefix: str, fi: FusedInput) -> None:
    """The index files and a .namesMap of NN rows (node v is "genome_v")."""
    oracle_lib.write_index(prefix, fi.color_off, fi.sources, fi.color_w, fi.group_ids, fi.kmer_counts)
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{fi.NN}\n")
        for i in range(fi.NN):
            f.write(f"{i + 1} genome_{i + 1}\n")


def reference(oracle_lib, prefix: str):
    """(pairwise TSV, seqToKmersNo TSV) as the oracle writes them for the index at prefix; both files stay where they are."""
    oracle_lib.ref_pairwise(prefix, 1)
    with open(prefix + "_kSpider_pairwise.tsv", "rb") as f:
        tsv = f.read()
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "rb") as f:
        seq = f.read()
    return tsv, seq


def rows_of(tsv: bytes) -> list:
    return [r.split("\t") for r in tsv.decode().split("\n")[1:-1]]


def without_zero_rows(tsv: bytes) -> bytes:
    lines = tsv.decode().split("\n")
    return "\n".join(lines[:1] + [l for l in lines[1:] if not l or l.split("\t")[2] != "0"]).encode()


def quartiles(rows: list, col: int) -> list:
    """The printed values at 1/4, 1/2 and 3/4 of the sorted distinct finite values of the column (fewer when there are fewer)."""
    distinct = sorted({r[col] for r in rows if math.isfinite(float(r[col]))}, key=float)
    picks = []
    for q in (1, 2, 3):
        if distinct:
            v = float(distinct[len(distinct) * q // 4])
            if v not in picks:
                picks.append(v)
    return picks


def cutoffs(rows: list, col: int, outside: bool) -> list:
    """The cut-offs of a column, from the reference TSV: its quartile values, the float above the middle one, 0 and 1 — and,
    for the calls that accept them, -1 (every row passes) and 2.0 (only NaN rows pass)."""
    picks = quartiles(rows, col)
    out = list(picks)
    if picks:
        out.append(float(np.nextafter(picks[len(picks) // 2], 2.0)))
    for c in (0.0, 1.0) + ((-1.0, 2.0) if outside else ()):
        if c not in out:
            out.append(c)
    return out


def derep_thresholds(rows: list, col: int) -> list:
    """The thresholds of the dereplication calls for a column, from the reference TSV: its quartile values, the float above
    the middle one (as `cutoffs` makes it), then 0.0, 0.20, 1.0 (above every finite value), 2.0 (only an infinite value passes)
    and +inf (nothing passes).  No negative one: the calls refuse them."""
    picks = quartiles(rows, col)
    out = list(picks)
    if picks:
        out.append(float(np.nextafter(picks[len(picks) // 2], 2.0)))
    for t in (0.0, 0.20, 1.0, 2.0, math.inf):
        if t not in out:
            out.append(t)
    return out


def names_beyond(rows: list, col: int, t: float, n_names: int) -> bool:
    """A row that passes the text test at t names an id above n_names: what kspider_dereplicate refuses."""
    import repr_restate as rr
    return any(rr.text_passes(r[col], t) and max(int(r[0]), int(r[1])) > n_names for r in rows)


def unsure_cut(rows: list) -> float:
    """The column-3 cut at which the `unsure` pairs are looked at: the middle quartile value."""
    picks = quartiles(rows, 3)
    return picks[len(picks) // 2]


# the (shape, seed)s both test files use: chosen so that tests/test_fused_inputs_cpu.py holds for the reference alone
CASES = (("tiny", 1), ("tiny", 5), ("mixed", 1), ("mixed", 2), ("mixed", 3), ("one_edge", 1), ("no_counts", 1), ("all_zero", 1))

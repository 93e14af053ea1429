"""What tests/test_fused_random_gpu.py relies on, shown with the oracle alone: per (shape, seed) of fused_inputs.CASES the index is
written, oracle.ref_pairwise writes the TSV, and the rows that make the GPU test mean something are counted there — rows that
exist only with shared_kmers = 0 in both NaN positions, infinite values, zero pairs that are real rows, the cut's `unsure`
pairs, components and a ranking that differ with and without the shared-0 rows, and cut-offs that cut; and, for the "derep" kind,
what tests/derep_restate.py makes of that TSV: rows of degree 0 with and without a source interleaved by id, more kept rows than
one chunk, members with a choice of representatives, rank ties, members through an infinite value."""
import os
import shutil

import numpy as np
import pytest

import cut_restate as cr
import derep_restate as dr
import fused_inputs as fz
import repr_restate as rr
from kspider_amd import engine
from oracle import ref_cluster


def _is_nan(text):
    return "nan" in text


@pytest.fixture(scope="module")
def cases(oracle_lib, tmp_path_factory):
    out = {}
    for shape, seed in fz.CASES:
        d = tmp_path_factory.mktemp(f"{shape}_{seed}")
        fi = fz.make(seed, shape)
        prefix = str(d / "ix")
        fz.write(oracle_lib, prefix, fi)
        tsv, seq = fz.reference(oracle_lib, prefix)
        out[shape, seed] = dict(fi=fi, dir=d, prefix=prefix, tsv=tsv, seq=seq, rows=fz.rows_of(tsv))
    return out


def _zero_pairs(fi):
    pairs = set()
    for c in range(len(fi.color_w)):
        members = sorted(fi.sources[fi.color_off[c]:fi.color_off[c + 1]].tolist())
        if fi.color_w[c] == 0:
            pairs.update((a, b) for i, a in enumerate(members) for b in members[i + 1:])
    return pairs


@pytest.mark.parametrize("shape,seed", fz.CASES)
def test_the_generator_is_seeded_and_shaped(cases, shape, seed):
    fi, again = cases[shape, seed]["fi"], fz.make(seed, shape)
    for name in ("color_off", "sources", "color_w", "group_ids", "kmer_counts"):
        assert (getattr(fi, name) == getattr(again, name)).all(), name
    other = fz.make(seed + 100, shape)
    assert other.ids != fi.ids or len(other.sources) != len(fi.sources) or (other.sources != fi.sources).any()
    assert fi.NN not in fi.ids and max(fi.ids) < fi.NN and sorted(set(fi.sources.tolist())) == fi.ids
    assert len(fi.ids) < fi.NN and fi.ids != list(range(1, len(fi.ids) + 1))                    # sparse ids, a longer .namesMap
    n, weights = len(fi.ids), fi.color_w
    if shape == "mixed":
        sizes = np.diff(fi.color_off.astype(np.int64))
        assert n == 120 and 1.25 * n <= fi.NN <= 1.35 * n and 400 <= len(weights) <= 800
        assert (weights == 0).mean() >= 0.25 and 40 in sizes[weights == 0] and 70 in sizes[weights > 0]
        assert ((sizes >= 2) & (sizes <= 5)).sum() >= 300
        sets = {}
        for c in range(len(weights)):
            sets.setdefault(tuple(sorted(fi.sources[fi.color_off[c]:fi.color_off[c + 1]].tolist())), set()).add(int(weights[c]))
        assert sum(len(w) >= 2 for w in sets.values()) >= 10                                    # a member set with two weights
        counts = dict(zip(fi.group_ids.tolist(), fi.kmer_counts.tolist()))
        zero = [g for g in fi.ids if counts.get(g, 0) == 0]
        assert 0.08 * n <= len(zero) <= 0.13 * n and len(fi.no_count) == 1 and fi.no_count[0] in fi.ids
        assert len(fi.zero_only) >= 2 and len(fi.single_only) >= 1 and len(fi.unsure) >= 3 and len(fi.zero_bridges) == 2
        for s in fi.zero_only + fi.single_only:
            for c in range(len(weights)):
                if s in fi.sources[fi.color_off[c]:fi.color_off[c + 1]]:
                    assert sizes[c] == 1 if s in fi.single_only else weights[c] == 0
    elif shape in ("tiny", "no_counts"):
        assert 7 <= n <= 12
        assert (fi.kmer_counts == 0).all() == (shape == "no_counts")
    elif shape == "all_zero":
        assert n == 30 and (weights == 0).all() and (fi.kmer_counts == 0).any()
    else:
        sizes = np.diff(fi.color_off.astype(np.int64))
        assert (weights > 0).sum() == 1 and sizes[weights > 0].tolist() == [2] and (weights == 0).sum() >= 5


@pytest.mark.parametrize("shape,seed", [c for c in fz.CASES if c[0] == "mixed"])
def test_mixed_rows_the_gpu_test_relies_on(cases, shape, seed):
    case = cases[shape, seed]
    fi, rows = case["fi"], case["rows"]
    zero = [r for r in rows if r[2] == "0"]
    real = {(int(r[0]), int(r[1])): r for r in rows if r[2] != "0"}
    nan_min = [r for r in zero if _is_nan(r[3])]
    nan_avg_only = [r for r in zero if r[3] == "0" and r[5] == "0" and _is_nan(r[4])]
    plain = [r for r in zero if r[3:] == ["0", "0", "0"]]
    with_inf = [r for r in real.values() if "inf" in r[3:]]
    both = [p for p in _zero_pairs(fi) if p in real]
    print(f"{shape}/{seed}: {len(rows)} rows, {len(zero)} shared-0 ({len(nan_min)} NaN in min, {len(nan_avg_only)} NaN in avg only, "
          f"{len(plain)} plain), {len(with_inf)} real rows with inf, {len(both)} zero pairs that are real rows")
    assert len(zero) >= 20 and len(nan_min) >= 5 and len(nan_avg_only) >= 5 and len(plain) >= 5
    assert len(with_inf) >= 5 and len(both) >= 5
    assert len(zero) + len(both) == len(_zero_pairs(fi))                   # every zero pair is a row, once
    counts = dict(zip(fi.group_ids.tolist(), fi.kmer_counts.tolist()))
    sides = {(counts.get(int(r[0]), 0) == 0, counts.get(int(r[1]), 0) == 0) for r in zero}
    assert sides == {(False, False), (True, False), (False, True), (True, True)}
    inf_sides = {(counts.get(a, 0) == 0, counts.get(b, 0) == 0) for (a, b) in real}
    assert {(True, False), (False, True)} <= inf_sides                      # real rows with the 0 on either side
    # the `unsure` pairs: real rows whose column-3 text fails the cut, beside a zero pair whose row would be a NaN row
    cut = fz.unsure_cut(rows)
    assert len(fi.unsure) >= 3
    for pair in fi.unsure:
        assert pair in real and pair in _zero_pairs(fi) and counts[pair[1]] == 0
        assert real[pair][2] == "1" and not cr.keep(real[pair][3], cut), (pair, real[pair], cut)
    # the zero-only rows that alone connect two components: one an ordinary 0-valued row, one a NaN row
    by_pair = {(int(r[0]), int(r[1])): r for r in zero}
    assert by_pair[fi.zero_bridges[0]][3:] == ["0", "0", "0"] and all(_is_nan(t) for t in by_pair[fi.zero_bridges[1]][3:])
    # ... so the cluster files with and without the shared-0 rows differ, at a cut-off the GPU test uses
    bare = case["dir"] / "bare"
    bare.mkdir()
    for ext in (".namesMap", "_kSpider_seqToKmersNo.tsv"):
        shutil.copy(case["prefix"] + ext, str(bare / "ix") + ext)
    with open(str(bare / "ix") + "_kSpider_pairwise.tsv", "wb") as f:
        f.write(fz.without_zero_rows(case["tsv"]))
    for dist, col in fz.DISTS.items():
        differs = []
        for c in fz.cutoffs(rows, col, outside=True):
            a, b = ref_cluster.write_clusters(case["prefix"], dist, c), ref_cluster.write_clusters(str(bare / "ix"), dist, c)
            differs.append(open(a, "rb").read() != open(b, "rb").read())
            os.remove(a), os.remove(b)
        assert any(differs) and differs[fz.cutoffs(rows, col, outside=True).index(0.0)], (dist, differs)
    # ... and the ranking at threshold -1 orders two ids differently (not only other counts)
    lo, hi = fi.rank_flip
    for col in (3, 4, 5):
        full = [int(l.split(b":")[0]) for l in rr.repr_sketches(case["tsv"].decode(), col, -1.0).split(b"\n") if l]
        part = [int(l.split(b":")[0]) for l in rr.repr_sketches(fz.without_zero_rows(case["tsv"]).decode(), col, -1.0).split(b"\n") if l]
        assert part.index(lo) < part.index(hi) and full.index(hi) < full.index(lo), col


@pytest.mark.parametrize("shape,seed", fz.CASES)
def test_cutoffs_cut(cases, shape, seed):
    """The quartile cut-offs keep between 5 % and 95 % of the rows ("mixed", "tiny"; the other shapes have at most two distinct
    finite values per column: their cut-offs are those, 0, 1, -1 and 2.0); every shape has rows with shared_kmers = 0."""
    rows, fi = cases[shape, seed]["rows"], cases[shape, seed]["fi"]
    assert any(r[2] == "0" for r in rows)
    assert any(_is_nan(t) for r in rows for t in r[3:])
    for dist, col in fz.DISTS.items():
        picks = fz.quartiles(rows, col)
        cs = fz.cutoffs(rows, col, outside=True)
        assert len(set(cs)) == len(cs) and {0.0, 1.0, -1.0, 2.0} <= set(cs)
        kept = {c: sum(cr.keep(r[col], c) for r in rows) for c in cs}
        print(f"{shape}/{seed} {dist}: {len(rows)} rows, kept {kept}")
        assert kept[-1.0] == kept[0.0] == len(rows)
        assert kept[2.0] == sum(_is_nan(r[col]) or r[col] == "inf" for r in rows)      # (only a NaN or an infinite value passes 2.0)
        if shape in ("mixed", "tiny"):
            assert len(picks) == 3
            for c in picks:
                assert 0.05 * len(rows) <= kept[c] <= 0.95 * len(rows), (dist, c, kept[c], len(rows))
            up = cs[3]
            assert up > picks[1] and kept[up] <= kept[picks[1]]             # (x 100 in double may round the two to one threshold)
    if shape == "tiny":
        cut = fz.unsure_cut(rows)
        (a, b), = fi.unsure
        row = next(r for r in rows if (int(r[0]), int(r[1])) == (a, b))
        assert row[2] == "1" and not cr.keep(row[3], cut)
        assert any(r[2] == "0" and _is_nan(r[3]) for r in rows)                 # a NaN row: what the ANI calls refuse
    if shape == "all_zero":
        assert all(r[2] == "0" for r in rows)
    if shape == "one_edge":
        assert sum(r[2] != "0" for r in rows) == 1
    if shape == "no_counts":
        assert all(_is_nan(t) or t == "inf" for r in rows for t in r[3:])


@pytest.mark.parametrize("shape,seed", [c for c in fz.CASES if c[0] in ("mixed", "tiny")])
def test_variant_with_counts_has_no_nan_row(cases, oracle_lib, shape, seed):
    """The index of the ANI calls: every source given a count, so no value is a NaN or an infinity, none above 1."""
    fi = fz.with_counts(cases[shape, seed]["fi"])
    d = cases[shape, seed]["dir"] / "counted"
    d.mkdir()
    fz.write(oracle_lib, str(d / "ix"), fi)
    tsv, _ = fz.reference(oracle_lib, str(d / "ix"))
    rows = fz.rows_of(tsv)
    assert len(rows) == len(cases[shape, seed]["rows"]) and any(r[2] == "0" for r in rows)
    assert all(0.0 <= float(t) <= 1.0 for r in rows for t in r[3:])


def _derep(case, dist, t):
    """(kept rows of the oracle TSV, the rows of the restatement's file as dicts) for a distance and a threshold."""
    fi, col = case["fi"], fz.DISTS[dist]
    names = [f"genome_{i + 1}" for i in range(fi.NN)]
    out = dr.dereplicated_tsv(case["tsv"].decode(), names, col, t, dist).decode().split("\n")
    assert out[0] == f"source\trepresentative\t{dist}\tneighbours\trank" and out[-1] == "" and len(out) == fi.NN + 2
    table = []
    for v, line in enumerate(out[1:-1]):
        name, rep, text, degree, rank = line.split("\t")
        assert name == names[v]
        table.append(dict(id=v + 1, rep=int(rep[len("genome_"):]), text=text, degree=int(degree), rank=int(rank)))
    assert sorted(r["rank"] for r in table) == list(range(fi.NN))
    return [r for r in case["rows"] if rr.text_passes(r[col], t)], table


def _between(flags):
    """Some True entry lies between two False ones."""
    return any(f and False in flags[:i] and False in flags[i + 1:] for i, f in enumerate(flags))


@pytest.mark.parametrize("shape,seed", fz.CASES)
def test_dereplication_rows_the_gpu_test_relies_on(cases, shape, seed):
    """Inequalities on the restatement of the oracle's TSV, per shape: what makes the "derep" kind of
    tests/test_fused_random_gpu.py exercise the finisher's renumbering of the degree-0 rows, the device's chunk loop, the
    assignment's choice, the id tie-break of the ranks and the infinite values."""
    case = cases[shape, seed]
    fi, NN = case["fi"], case["fi"].NN
    is_rep = lambda r: r["rep"] == r["id"]
    for dist, col in fz.DISTS.items():
        ladder = fz.derep_thresholds(case["rows"], col)
        assert {0.0, 0.20, 1.0, 2.0} <= set(ladder) and ladder[-1] == float("inf") and len(set(ladder)) == len(ladder) and min(ladder) >= 0
        # degree-0 rows of sources and rows without a source, interleaved by id in both ways
        kept, table = _derep(case, dist, 0.20)
        lone = [r["id"] in fi.ids for r in table if r["degree"] == 0]
        print(f"{shape}/{seed} {dist} at 0.20: {len(kept)} kept, {sum(lone)} degree-0 sources, {len(lone) - sum(lone)} rows without a source")
        assert _between(lone) and _between([not f for f in lone]), dist
        assert all(is_rep(r) and r["text"] == "-" for r in table if r["degree"] == 0)
        kept, table = _derep(case, dist, float("inf"))
        assert not kept and all(is_rep(r) for r in table) and [r["rank"] for r in table] == list(range(NN))
        if shape == "mixed":
            kept, table = _derep(case, dist, 0.0)
            reps = {r["id"] for r in table if is_rep(r)}
            nbrs = {}
            for r in kept:
                a, b = int(r[0]), int(r[1])
                nbrs.setdefault(a, set()).add(b)
                nbrs.setdefault(b, set()).add(a)
            choice = sum(len(nbrs[r["id"]] & reps) >= 2 for r in table if not is_rep(r))
            degrees = [r["degree"] for r in table if r["degree"] > 0]
            print(f"{shape}/{seed} {dist} at 0.0: {len(kept)} kept, {len(reps)} representatives of {NN}, {choice} members with a choice, "
                  f"largest degree {max(degrees)}")
            assert len(kept) > engine.DEREP_CHUNK_EDGES
            assert NN / 4 <= len(reps) <= NN / 2
            assert choice >= 20
            assert len(set(degrees)) < len(degrees)                                  # two sources of one degree: the id breaks the tie
            if dist == "min_cont":
                assert 1 <= len(_derep(case, dist, 0.20)[0]) <= 50
            else:
                kept, table = _derep(case, dist, 2.0)
                assert len(kept) >= 100 and all(r[col] == "inf" for r in kept)
                assert sum(r["text"] == "inf" for r in table) >= 50
            # what the GPU test reads from the written file at 0.0: the planted ids
            assert fi.rank_flip[0] in fi.ids and set(range(1, NN + 1)) - set(fi.ids)
    if shape == "tiny":
        assert any(r["text"] == "inf" for dist, col in fz.DISTS.items() for t in fz.derep_thresholds(case["rows"], col)
                   for r in _derep(case, dist, t)[1])
    if shape == "no_counts":
        for dist, col in fz.DISTS.items():
            at0, at2 = _derep(case, dist, 0.0)[0], _derep(case, dist, 2.0)[0]
            assert at0 and at0 == at2 and all(r[col] == "inf" for r in at0)
    if shape == "one_edge":
        for dist, col in fz.DISTS.items():
            kept, table = _derep(case, dist, 0.0)
            assert len(kept) == 1 and sum(not is_rep(r) for r in table) == 1
            above = float(np.nextafter(np.float32(rr.strtof(kept[0][col])), np.float32(2.0)))
            ladder = fz.derep_thresholds(case["rows"], col)
            up = min(t for t in ladder if t >= above)
            assert up < float("inf") and all(is_rep(r) for r in _derep(case, dist, up)[1])
    if shape == "all_zero":
        for dist in fz.DISTS:
            kept, table = _derep(case, dist, 0.0)
            assert not kept and all(is_rep(r) for r in table) and [r["rank"] for r in table] == list(range(NN))


def test_a_short_names_map_gives_both_outcomes_on_a_tiny_case(cases):
    """.namesMap cut to one row fewer than the largest source id, as tests/test_fused_random_gpu.py cuts it: on one "tiny" case at
    least a passing row names the missing id at some threshold of the ladder and none does at another.  (On "tiny" seed 1 the
    largest id has rows with shared_kmers = 0 only, which pass no threshold >= 0: that case shows the second outcome alone.)"""
    both = 0
    for (shape, seed), case in cases.items():
        if shape == "tiny":
            short = max(case["fi"].ids) - 1
            seen = {fz.names_beyond(case["rows"], col, t, short) for col in fz.DISTS.values() for t in fz.derep_thresholds(case["rows"], col)}
            assert False in seen
            both += seen == {True, False}
    assert both >= 1

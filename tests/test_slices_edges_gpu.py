"""The sliced stage 1 (build_slice / build_postings_slice ... assemble) at its cuts, its limits and in the engine's
modes.  Every case compares the whole edge set with a reference (a closed form, the brute-force oracle, the oracle's
weighted accumulation, or the unsliced run and one of those) and proves what the slices held: slice_sizes()[1], the
distinct shared keys of a slice, against the restatement of the cut (tests/slice_inputs.py), and their sum against
n_kept_keys of the unsliced build — a key built in two slices shows there even where the join would hide it."""
import numpy as np
import pytest

import edge_inputs as E
import slice_inputs as S
from kspider_amd import engine
from pair_probe import check_edge_set, config, sort_edges
from slice_driver import Sketches, sliced_edges, sliced_postings_edges
from test_fuzz_gpu import _random_sketches
from test_thresholds_gpu import KNOBS, _weighted_ref

pytestmark = pytest.mark.gpu

ALL_KNOBS = KNOBS + ("KSP_SLICES",)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _env(monkeypatch, env):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _same(edges, ref, what):
    assert len(edges) == len(ref), (what, len(edges), len(ref))
    assert (edges["source_1"] == ref["source_1"]).all() and (edges["source_2"] == ref["source_2"]).all(), what
    bad = np.flatnonzero(edges["shared"] != ref["shared"])
    assert bad.size == 0, (what, "counts differ", edges[bad[:4]], ref[bad[:4]])


def _check_slices(keys, offsets, nparts, want, what, weights=None, key_bits=0, devices=True):
    """The slice driver (and, where the engine derives the span itself, pairwise_host on nparts workers) on this input:
    edges equal `want` and the unsliced run; every slice held the shared keys of its part of [0, span).
    (pairwise_host takes no key_bits, so the fixed-width cases go through the driver only; devices=False is passed
    where the case also runs pairwise_host under KSP_SLICES = nparts, which run_multi turns into devices = [0] * nparts:
    the same path.)"""
    sk = Sketches(keys, offsets)
    one, st1 = engine.pairwise_host(keys, offsets, weights)
    _same(one, want, (what, "unsliced"))
    edges, sizes, st = sliced_edges(sk, nparts, weights, key_bits)
    kept = sizes[1::4].astype(np.int64)
    ref = S.kept_keys_per_part(keys, S.engine_span(keys, key_bits), nparts)
    print(what, "kept keys per slice", kept.tolist(), "restated", ref.tolist(), "unsliced", st1["n_kept_keys"])
    assert (kept == ref).all(), (what, "shared keys per slice", kept.tolist(), ref.tolist())
    assert int(kept.sum()) == st1["n_kept_keys"] == st["n_kept_keys"], (what, kept.tolist(), st1["n_kept_keys"])
    _same(edges, want, (what, "slice driver"))
    if key_bits == 0 and devices:
        many, stm = engine.pairwise_host(keys, offsets, weights, devices=[0] * nparts)
        _same(many, want, (what, "devices"))
        if len(want):
            assert stm["n_kept_keys"] == st1["n_kept_keys"], (what, stm["n_kept_keys"], st1["n_kept_keys"])
    return sizes, st


# ---- A. the key-range cut ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [(1 << 20) + 1, 1 << 63, 1 << 64])
@pytest.mark.parametrize("nparts", [2, 3, 7, 64])
def test_keys_on_every_cut(span, nparts):
    """Keys lo, lo + 1, end - 2, end - 1 of every part, each held by a pair of its own: the span comes from the largest
    key (span - 1)."""
    keys, offsets, want, kept = S.cut_input(span, nparts)
    assert int(keys.max()) == span - 1 and (kept >= 4).all()
    sizes, _ = _check_slices(keys, offsets, nparts, want, ("cuts", span, nparts))
    assert (sizes[1::4] == kept).all()
    # few sources: every pair holds keys of several parts (shared = keys given to the pair)
    keys, offsets, want, kept = S.cut_input(span, nparts, n_sources=12)
    assert int(want["shared"].max()) > 1
    _check_slices(keys, offsets, nparts, want, ("cuts, 6 pairs", span, nparts))


@pytest.mark.parametrize("key_bits", [40, 64])
@pytest.mark.parametrize("nparts", [2, 3, 7, 64])
def test_keys_on_every_cut_of_a_fixed_key_width(key_bits, nparts):
    """The caller fixes key_bits: span = 2^key_bits.  All parts filled; then the top parts empty (largest key far below
    the span), the first part empty, and every part but one empty."""
    span = 1 << key_bits
    keys, offsets, want, kept = S.cut_input(span, nparts)
    sizes, _ = _check_slices(keys, offsets, nparts, want, ("fixed", key_bits, nparts), key_bits=key_bits)
    assert (sizes[1::4] == kept).all() and (kept >= 4).all()
    top_empty = tuple(range((nparts + 1) // 2, nparts))
    for empty in (top_empty, (0,) + top_empty[1:], tuple(p for p in range(nparts) if p != nparts // 2)):
        keys, offsets, want, kept = S.cut_input(span, nparts, empty_parts=empty)
        assert len(want) and all(kept[p] == 0 for p in empty)
        sizes, _ = _check_slices(keys, offsets, nparts, want, ("fixed", key_bits, nparts, empty), key_bits=key_bits)
        assert (sizes[1::4] == kept).all()


@pytest.mark.parametrize("span", [1, 2, 3])
@pytest.mark.parametrize("nparts", [2, 3, 8])
@pytest.mark.parametrize("holders", [2, 3])
def test_fewer_keys_than_slices(oracle_lib, span, nparts, holders):
    """Keys 0 .. span - 1 only (colour ids fed as keys): with span < nparts some parts have no key at all.  Unweighted
    and weighted (a key built in two slices doubles its weight in `shared`)."""
    keys, offsets, who = S.small_span_input(span, holders)
    want = S.pairs_from_holders(who)
    ref = oracle_lib.brute_pairs(keys, offsets)
    assert (ref == want).all() and int(keys.max()) == span - 1
    _check_slices(keys, offsets, nparts, want, ("small span", span, nparts, holders))
    wk = {k: 1000 + 7 * k for k in who}
    w = np.array([wk[int(k)] for k in keys], dtype=np.uint32)
    wwant = S.pairs_from_holders(who, wk)
    assert (_weighted_ref(oracle_lib, keys, offsets, w) == wwant).all()
    _check_slices(keys, offsets, nparts, wwant, ("small span, weighted", span, nparts, holders), weights=w)


def test_two_sources_one_key_zero_on_two_devices():
    """[[0], [0]]: span 1, two slices — the smallest input of the kind above."""
    keys, offsets = S.arrays([[0], [0]])
    two, _ = engine.pairwise_host(keys, offsets, devices=[0, 0])
    _same(two, S.edges_of({(0, 1): 1}), "[[0], [0]]")


@pytest.mark.parametrize("nparts", [2, 3, 8])
def test_one_key_per_slice(oracle_lib, nparts):
    """span == nparts (one key per part) and span == nparts + 1 (one part holds two)."""
    for span in (nparts, nparts + 1):
        widths = [end - lo for lo, end in S.key_cuts(span, nparts)]
        assert sorted(widths) == [1] * (nparts - (span - nparts)) + [2] * (span - nparts)
        keys, offsets, who = S.small_span_input(span, 3)
        want = S.pairs_from_holders(who)
        assert (oracle_lib.brute_pairs(keys, offsets) == want).all()
        sizes, _ = _check_slices(keys, offsets, nparts, want, ("span", span, nparts))
        assert sizes[1::4].tolist() == widths


def test_runs_and_slices(oracle_lib):
    """4 parts of [0, 4000): the first part empty; a source whose whole run lies in one part; a source with an empty
    run; a source whose run starts exactly at lo_p and ends exactly at end_p - 1; a source with one key per part."""
    span, nparts = 4000, 4
    cuts = S.key_cuts(span, nparts)
    assert cuts == [(0, 1000), (1000, 2000), (2000, 3000), (3000, 4000)]
    exact = list(range(2000, 3000))                 # lo_2 .. end_2 - 1
    inside = list(range(1400, 1500))                # all in part 1
    runs = [exact, [], inside, [1000, 1450, 1999, 2000, 2999, 3000, 3999], exact[::2] + [3999], [1499, 1500, 2500],
            [], [3000, 3001, 3998, 3999], [1000, 2999], inside[5:50] + [3500]]
    keys, offsets = S.arrays(runs)
    assert int(keys.min()) == 1000 and int(keys.max()) == span - 1      # nothing in part 0, the span from key 3 999
    want = oracle_lib.brute_pairs(keys, offsets)
    sizes, _ = _check_slices(keys, offsets, nparts, want, "runs")
    assert sizes[1] == 0 and (sizes[5::4] > 0).all()
    # every part but the last empty: key 3 999 stretches the span, all other keys sit next to it
    runs = [[3990, 3999], [3990, 3998, 3999], [], [3998]]
    keys, offsets = S.arrays(runs)
    want = oracle_lib.brute_pairs(keys, offsets)
    sizes, _ = _check_slices(keys, offsets, nparts, want, "all in the last part")
    assert sizes[1::4].tolist() == [0, 0, 0, 3]


# ---- B. the assemble across slices that differ in structure ----------------------------------------------------------
def _three_part_keys(per_part):
    """Key values for 3 parts of [0, 3 x 2^20): per_part[p] keys spread inside part p (and key 3 x 2^20 - 1 exists)."""
    span = 3 << 20
    out = []
    for p, n in enumerate(per_part):
        lo, end = S.key_cuts(span, 3)[p]
        ks = [lo + 1 + (i * 7919) % (end - lo - 2) for i in range(n)]
        assert len(set(ks)) == n
        out.append(ks)
    return span, out


def test_masks_in_slices_around_a_slice_without(oracle_lib, monkeypatch):
    """Keys with more than INLINE_MAX holders in a block (a mask each) in parts 0 and 2, in different numbers, and only
    two-holder keys in part 1: the mask offset of part 2 counts part 0's masks across a part that has none.  Holder
    counts per block as in test_inline_max_holders / test_dense_max_holders."""
    span, ks = _three_part_keys([3, 40, 4])
    n = 256
    runs = [[] for _ in range(n)]
    who = {}

    def hold(key, ha, hb):
        who[key] = list(range(ha)) + list(range(128, 128 + hb))
        for s in who[key]:
            runs[s].append(key)

    for key, (ha, hb) in zip(ks[0], [(5, 0), (6, 49), (3, 48)]):
        hold(key, ha, hb)
    for key, (ha, hb) in zip(ks[2], [(47, 5), (5, 5), (1, 6), (49, 2)]):
        hold(key, ha, hb)
    for i, key in enumerate(ks[1]):
        who[key] = [(3 * i) % n, (3 * i + 131) % n]
        for s in who[key]:
            runs[s].append(key)
    runs[n - 1].append(span - 1)                     # the span: 3 x 2^20
    runs[n - 2].append(span - 1)
    who[span - 1] = [n - 2, n - 1]
    keys, offsets = S.arrays(runs)
    assert (S.part_of(np.array(ks[0]), span, 3) == 0).all() and (S.part_of(np.array(ks[1]), span, 3) == 1).all()
    assert (S.part_of(np.array(ks[2] + [span - 1]), span, 3) == 2).all()
    want = S.pairs_from_holders(who)
    assert (oracle_lib.brute_pairs(keys, offsets) == want).all()
    for env in ({"KSP_REORDER": "0"}, {"KSP_REORDER": "0", "KSP_JOIN": "window"}, {"KSP_REORDER": "0", "KSP_JOIN": "matches"}, {}):
        _env(monkeypatch, env)
        sizes, st = _check_slices(keys, offsets, 3, want, ("masks", env))
        nbig = sizes[2::4].tolist()
        print("masks per slice", env, nbig)
        if env.get("KSP_REORDER") == "0":   # blocks = source // 128: the masks are where the input put them
            assert st["n_blocks"] == 2
            assert nbig[1] == 0 and nbig[0] > 0 and nbig[2] > 0 and nbig[0] != nbig[2], nbig


def test_key_with_thousands_of_holders_in_the_last_slice():
    span, ks = _three_part_keys([30, 30, 1])
    n, h = 2600, 2500
    runs = [[] for _ in range(n)]
    big = ks[2][0]
    for s in range(h):
        runs[s].append(big)
    want = {}
    for i, key in enumerate(ks[0] + ks[1]):          # two-holder keys: pairs (2i, 2i + 1) inside the big key's holders
        a = 2 * i if i < 40 else h + 2 * (i - 40)    # ... and 20 pairs outside them
        runs[a].append(key)
        runs[a + 1].append(key)
        want[(a, a + 1)] = 1
    runs[n - 1].append(span - 1)
    keys, offsets = S.arrays(runs)
    s1, s2 = np.triu_indices(h, 1)
    ref = np.zeros(s1.size, dtype=engine.EDGE_DTYPE)
    ref["source_1"], ref["source_2"], ref["shared"] = s1, s2, 1
    ref["shared"][(s2 == s1 + 1) & (s1 % 2 == 0) & (s1 < 80)] = 2
    extra = S.edges_of({p: c for p, c in want.items() if p[0] >= h})
    ref = sort_edges(np.concatenate([ref, extra]))
    sizes, _ = _check_slices(keys, offsets, 3, ref, "thousands of holders")
    assert sizes[1::4].tolist() == [30, 30, 1]


@pytest.mark.parametrize("total", [65535, 65536, 65537])
def test_weight_sums_on_the_16_bit_edge_across_slices(oracle_lib, monkeypatch, total):
    """test_counter_width_weighted with its three keys in three different slices: the 32-bit decision is taken after
    the assemble, from sums no single slice saw."""
    k3 = [1, 50, 100]
    assert S.part_of(np.array(k3), 101, 3).tolist() == [0, 1, 2]
    runs = [[] for _ in range(129)]
    runs[0] = list(k3)
    runs[128] = list(k3)
    keys, offsets = S.arrays(runs)
    w3 = [total // 3, total // 3, total - 2 * (total // 3)]
    w = np.array(w3 + w3, dtype=np.uint32)
    want = S.edges_of({(0, 128): total})
    assert (_weighted_ref(oracle_lib, keys, offsets, w) == want).all()
    for env in ({"KSP_REORDER": "0"}, {"KSP_REORDER": "0", "KSP_NO_SCHED": "1"}, {"KSP_REORDER": "0", "KSP_KEY_GROUPS": "0"}, {}):
        _env(monkeypatch, env)
        sizes, st = _check_slices(keys, offsets, 3, want, ("weighted 16-bit edge", total, env), weights=w)
        assert st["weighted"] and sizes[1::4].tolist() == [1, 1, 1]


@pytest.mark.parametrize("k", [65535, 65536, 65537, 2 * 65535])
@pytest.mark.parametrize("b", [128, 1])
def test_counter_width_on_assembled_lists(monkeypatch, k, b):
    """A pair sharing k keys spread over 2 and 3 slices: counter width and share cutting on assembled lists."""
    keys, offsets = E.pair_input(k, 129, 0, b)
    want = S.edges_of({(0, b): k})
    for nparts in (2, 3):
        kept = S.kept_keys_per_part(keys, k + 1, nparts)
        assert kept.sum() == k and kept.min() >= k // nparts - 1
        for env in ({}, {"KSP_JOIN": "matches"}, {"KSP_JOIN": "window"}, {"KSP_COLLECT": "0"},
                    {"KSP_JOIN": "matches", "KSP_DEBUG_NO16CUT": "1"}, {"KSP_JOIN": "window", "KSP_NO_SCHED": "1"}):
            _env(monkeypatch, dict(env, KSP_REORDER="0", KSP_SLICES=nparts))
            edges, st = engine.pairwise_host(keys, offsets)
            _same(edges, want, (k, b, nparts, env))
            assert st["n_blocks"] == 2 and st["n_kept_keys"] == k, st
            # assembled lists have no match records (KSP_JOIN): the whole build has k of them, the slices none
            assert st["n_match_records"] == 0, (env, st)
            if env.get("KSP_JOIN") == "matches" and b == 128:
                _env(monkeypatch, dict(env, KSP_REORDER="0"))
                _, stw = engine.pairwise_host(keys, offsets)
                assert stw["n_match_records"] == k, stw
        _env(monkeypatch, {"KSP_REORDER": "0"})
        sizes, _ = _check_slices(keys, offsets, nparts, want, ("counter width", k, b, nparts), devices=False)
        assert (sizes[1::4] == kept).all()


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_source_tags_width_in_two_slices(monkeypatch, n):
    """test_source_tags_width's input in 2 slices: u16 / u32 tags in k_range_copy."""
    src = np.arange(n, dtype=np.uint64)
    pair_key = (src // 2) * 4 + 10
    first = np.array([1, 2, 3], dtype=np.uint64)
    rs = [np.sort(np.concatenate([first, pair_key[s:s + 1]])) if s in (0, n - 1) else pair_key[s:s + 1] for s in range(n)]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in rs])
    keys = np.concatenate(rs)
    rows = {(2 * i, 2 * i + 1): 1 for i in range(n // 2)}
    rows[(0, n - 1)] = rows.get((0, n - 1), 0) + 3
    want = S.edges_of(rows)
    for env in ({}, {"KSP_TAG32": "1"}):
        _env(monkeypatch, dict(env, KSP_SLICES=2))
        edges, st = engine.pairwise_host(keys, offsets)
        _same(edges, want, (n, env))
        assert st["n_sources"] == n, st
    _env(monkeypatch, {})
    _check_slices(keys, offsets, 2, want, ("source tags", n), devices=False)


@pytest.mark.parametrize("nb", [257, 1025])
def test_block_tables_of_the_assemble(monkeypatch, nb):
    """nb blocks of 128 sources (KSP_ALIGN=0: plain cuts) in 3 slices: sources in groups of 8 share 4 keys of their
    own, and a few keys are shared across distant blocks."""
    n = 128 * nb
    src = np.arange(n, dtype=np.uint64)
    keys = ((src // 8)[:, None] * 4 + np.arange(4, dtype=np.uint64)[None, :] + 1).reshape(-1)
    top = n // 8 * 4 + 1                                 # first key above the groups' keys
    far = [(0, n - 1), (5, n // 2 + 3), (128 * 100 + 3, 128 * 200 + 7), (77, 128 * (nb - 1))]
    runs = keys.reshape(n, 4)
    lens = np.full(n, 4)
    extra = {}
    for j, (a, b) in enumerate(far):
        for s in (a, b):
            extra.setdefault(s, []).append(top + 10 * j)
            lens[s] += 1
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    out = np.zeros(int(offsets[-1]), dtype=np.uint64)
    for s in range(n):
        o = int(offsets[s])
        out[o:o + 4] = runs[s]
        if s in extra:
            out[o + 4:o + lens[s]] = extra[s]
    keys = out
    g = np.arange(0, n, 8, dtype=np.int64)
    xs, ys = np.triu_indices(8, 1)
    want = np.zeros(g.size * xs.size + len(far), dtype=engine.EDGE_DTYPE)
    want["source_1"][:g.size * xs.size] = (g[:, None] + xs[None, :]).reshape(-1)
    want["source_2"][:g.size * xs.size] = (g[:, None] + ys[None, :]).reshape(-1)
    want["shared"] = 4
    for j, (a, b) in enumerate(far):
        want[g.size * xs.size + j] = (a, b, 1)
    want = sort_edges(want)
    for env in ({"KSP_ALIGN": "0"}, {"KSP_ALIGN": "0", "KSP_MS": "0"}, {}):
        _env(monkeypatch, dict(env, KSP_SLICES=3))
        edges, st = engine.pairwise_host(keys, offsets)
        _same(edges, want, (nb, env))
        if "KSP_ALIGN" in env:
            assert st["n_blocks"] == nb, st
        assert st["n_kept_keys"] == n // 8 * 4 + len(far), st
    _env(monkeypatch, {"KSP_ALIGN": "0"})
    sizes, st = _check_slices(keys, offsets, 3, want, ("blocks", nb), devices=False)
    assert st["n_blocks"] == nb


# ---- C. engine modes x slices ----------------------------------------------------------------------------------------
SLICE_MODES = [{}, {"KSP_REORDER": "0"}, {"KSP_NO_SCHED": "1"}, {"KSP_COLLECT": "0"}, {"KSP_COLLECT": "1"},
               {"KSP_JOIN": "window"}, {"KSP_JOIN": "matches"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "0"},
               {"KSP_JOIN": "matches", "KSP_COLLECT": "1"}, {"KSP_TAG32": "1"}, {"KSP_HASH_GROUP": "0"},
               {"KSP_KEY_GROUPS": "0"}, {"KSP_ALIGN": "0"}, {"KSP_MS": "0"}, {"KSP_FULL_SORT": "1"}]


def _shared_keys(keys):
    _, cnt = np.unique(keys, return_counts=True)
    return int((cnt >= 2).sum())


@pytest.mark.parametrize("seed", range(12))
def test_random_sketches_in_slices_all_modes(oracle_lib, seed, monkeypatch):
    rng = np.random.default_rng(1000 + seed)     # (test_fuzz_gpu's seeds: universes 8 and 60 among them)
    for _ in range(6):
        sk = _random_sketches(rng)
        ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
        _env(monkeypatch, {})
        _, st1 = engine.pairwise_host(sk.keys, sk.offsets)
        kept = _shared_keys(sk.keys)
        if len(ref):
            assert st1["n_kept_keys"] == kept, (seed, st1)

        def check(edges, st, what):
            assert len(edges) == len(ref) and (edges == ref).all(), (seed, what, sk.n_sources)
            if len(ref):   # every shared key was built in exactly one slice
                assert st["n_kept_keys"] == kept, (seed, what, st["n_kept_keys"], kept)
            # (KSP_JOIN=matches: assembled lists have no match records, the search join runs — DESIGN.md, KSP_JOIN)
            assert st["n_match_records"] == 0 and st["stage1_kind"] == 0 and st["partition_kind"] in (0, 1), (seed, what, st)

        for env in SLICE_MODES:
            for slices in (2, 5):
                _env(monkeypatch, dict(env, KSP_SLICES=slices))
                check(*engine.pairwise_host(sk.keys, sk.offsets), (env, slices))
            if seed < 3:
                _env(monkeypatch, env)
                check(*engine.pairwise_host(sk.keys, sk.offsets, devices=[0, 0, 0]), (env, "devices"))


def test_hand_partition_and_fused_stage1_stay_off_in_slices(oracle_lib, monkeypatch):
    """The hand-written partition and the bucket-resident stage 1 are whole-build paths (e->nparts == 1 in build_impl):
    asking for them with slices must leave them off, and the edges right."""
    rng = np.random.default_rng(77)
    runs = [np.unique(rng.integers(0, 1 << 30, size=60, dtype=np.uint64)) for _ in range(200)]
    fam = np.unique(rng.integers(0, 1 << 30, size=40, dtype=np.uint64))
    runs = [np.unique(np.concatenate([r, fam[rng.random(fam.size) < 0.5]])) for r in runs]
    keys, offsets = S.arrays([r.tolist() for r in runs])
    assert keys.size >= 4096
    ref = oracle_lib.brute_pairs(keys, offsets)
    for env in ({"KSP_PART_MIN": "1"}, {"KSP_FUSED": "1", "KSP_PART_MIN": "1", "KSP_JOIN": "window"}, {"KSP_PART_MIN": "1", "KSP_SEG": "1"}):
        _env(monkeypatch, env)
        edges, st = engine.pairwise_host(keys, offsets)
        _same(edges, ref, (env, "whole"))
        assert st["partition_kind"] in (2, 3), st      # (whole build: the hand-written partition engages)
        assert st["stage1_kind"] == int("KSP_FUSED" in env), st   # (... and the bucket-resident stage 1 where asked for)
        _env(monkeypatch, dict(env, KSP_SLICES=3))
        edges, st = engine.pairwise_host(keys, offsets)
        _same(edges, ref, (env, "slices"))
        assert st["partition_kind"] in (0, 1) and st["stage1_kind"] == 0, st
        _env(monkeypatch, env)
        edges, _, st = sliced_edges(Sketches(keys, offsets), 3)
        _same(edges, ref, (env, "driver"))
        assert st["partition_kind"] in (0, 1) and st["stage1_kind"] == 0, st


def _weighted_case(rng, sk):
    """test_fuzz_gpu's weighted half: ({pair: weight sum}, per-entry weights, postings of the shared keys)."""
    n = sk.n_sources
    src = np.repeat(np.arange(n, dtype=np.uint32), np.diff(sk.offsets).astype(np.int64))
    uniq, inv = np.unique(sk.keys, return_inverse=True)
    wkey = rng.integers(0, 1000, size=uniq.size, dtype=np.uint32)
    order = np.argsort(inv, kind="stable")
    ks, ss = inv[order], src[order]
    bounds = np.flatnonzero(np.diff(ks)) + 1
    groups = np.split(ss, bounds)
    gkeys = ks[np.concatenate([[0], bounds])]
    who = {int(kidx): g.tolist() for g, kidx in zip(groups, gkeys) if g.size >= 2}
    want = S.pairs_from_holders(who, wkey)
    return want, wkey[inv], who, wkey


@pytest.mark.parametrize("seed", range(6))
def test_random_weighted_and_postings_in_slices(seed, monkeypatch):
    """test_fuzz_gpu's weighted sketches and the same data as an inverted index, under KSP_SLICES = 2 and 5.  (Seed 3's
    index in 5 slices is where a source's weight sum passes 2^16 only over all slices together: see
    test_postings_slices_whose_bounds_pass_16_bits_only_together.)"""
    rng = np.random.default_rng(2000 + seed)
    for _ in range(4):
        sk = _random_sketches(rng)
        if sk.keys.size == 0:
            continue
        want, w, who, wkey = _weighted_case(rng, sk)
        perm = rng.permutation(len(who))
        kidx = list(who)
        key_off = np.zeros(len(who) + 1, dtype=np.uint64)
        key_off[1:] = np.cumsum([len(who[kidx[i]]) for i in perm])
        sources = np.concatenate([rng.permutation(who[kidx[i]]) for i in perm] + [np.zeros(0, np.int64)]).astype(np.uint32)
        wts = np.array([wkey[kidx[i]] for i in perm], dtype=np.uint32)
        for env in ({}, {"KSP_REORDER": "0"}, {"KSP_NO_SCHED": "1"}, {"KSP_KEY_GROUPS": "0"}):
            for slices in (2, 5):
                _env(monkeypatch, dict(env, KSP_SLICES=slices))
                edges, st = engine.pairwise_host(sk.keys, sk.offsets, w)
                _same(edges, want, (seed, env, slices, "weighted"))
                if len(who):
                    assert st["n_kept_keys"] == len(who) == _shared_keys(sk.keys), (seed, env, slices, st)
                    e2, st2 = engine.pairwise_postings_host(key_off, sources, wts, sk.n_sources)
                    _same(e2, want, (seed, env, slices, "postings"))
                    if len(who) >= slices:   # (fewer keys than slices: one whole build)
                        assert st2["n_kept_keys"] == len(who), (seed, env, slices, st2)


# ---- D. postings slices ----------------------------------------------------------------------------------------------
def _postings_input(counts, n_sources, seed=0, same_block=None):
    """Key k held by counts[k] random sources (same_block: keys whose holders are all below source 128)."""
    rng = np.random.default_rng(seed)
    who = {}
    for k, c in enumerate(counts):
        pool = min(128, n_sources) if same_block and k in same_block else n_sources
        who[k] = rng.choice(pool, size=int(c), replace=False).tolist()
    key_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sources = np.concatenate([np.array(who[k], dtype=np.uint32) for k in range(len(counts))])
    return key_off, sources, who


def _check_postings(monkeypatch, key_off, sources, who, n_sources, nd, what, env=None):
    """run_multi's own pk_cut is covered here through the edge sets of the KSP_SLICES / devices runs (the host entry reports
    no per-slice figure) and as numbers on the CPU (tests/test_slice_plan_cpu.py); the driver is handed the restatement's cuts, so its slice_sizes()[1] == keys per
    slice shows what that slot means for postings slices and that slices cut there assemble to the right result."""
    env = env or {}
    n_keys = key_off.size - 1
    cuts = S.postings_cuts(key_off, nd)
    for wts in (None, (np.arange(n_keys, dtype=np.uint32) * 37) % 900 + 1):
        want = S.pairs_from_holders(who, wts)
        _env(monkeypatch, env)
        one, st1 = engine.pairwise_postings_host(key_off, sources, wts, n_sources)
        _same(one, want, (what, "unsliced"))
        _env(monkeypatch, dict(env, KSP_SLICES=nd))
        forced, _ = engine.pairwise_postings_host(key_off, sources, wts, n_sources)
        _same(forced, want, (what, "KSP_SLICES"))
        _env(monkeypatch, env)
        many, _ = engine.pairwise_postings_host(key_off, sources, wts, n_sources, devices=[0] * nd)
        _same(many, want, (what, "devices"))
        edges, sizes, st = sliced_postings_edges(key_off, sources, wts, n_sources, cuts)
        _same(edges, want, (what, "driver", cuts))
        kept = sizes[1::4].astype(np.int64).tolist()
        print(what, "cuts", cuts, "keys per slice", kept)
        assert kept == [b - a for a, b in zip(cuts, cuts[1:])], (what, cuts, kept)
        assert sum(kept) == n_keys == st["n_kept_keys"], (what, kept, st)
    return cuts


@pytest.mark.parametrize("nd", [2, 3, 7])
def test_postings_slices_by_key_count(monkeypatch, nd):
    """n_keys == nd (one key each), nd + 1, and nd - 1 (more slices than keys: one build, by the documented rule)."""
    for n_keys in (nd, nd + 1, nd - 1):
        counts = [2 + (3 * k) % 5 for k in range(n_keys)]
        key_off, sources, who = _postings_input(counts, 300, seed=nd * 10 + n_keys)
        cuts = _check_postings(monkeypatch, key_off, sources, who, 300, nd, ("keys", n_keys, nd))
        if n_keys < nd:
            assert cuts == [0, n_keys]
        else:
            assert len(cuts) == nd + 1 and min(b - a for a, b in zip(cuts, cuts[1:])) >= 1


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_postings_slices_with_one_key_of_half_the_memberships(monkeypatch, where):
    small = [2 + k % 3 for k in range(120)]
    big = sum(small)
    at = {"first": 0, "middle": 60, "last": 120}[where]
    counts = small[:at] + [big] + small[at:]
    key_off, sources, who = _postings_input(counts, 400, seed=at)
    assert 2 * counts[at] == int(key_off[-1])
    for nd in (2, 3, 5):
        cuts = _check_postings(monkeypatch, key_off, sources, who, 400, nd, ("half", where, nd))
        s = next(i for i in range(nd) if cuts[i] <= at < cuts[i + 1])   # the slice of the big key
        print(where, nd, "the big key is in slice", s, cuts)
        if where == "first":
            assert cuts[1] == 1 if nd == 2 else s == 0


def test_postings_slices_of_two_holder_keys_and_a_slice_in_one_block(monkeypatch):
    counts = [2] * 600
    key_off, sources, who = _postings_input(counts, 500, seed=3)
    for nd in (2, 5):
        cuts = _check_postings(monkeypatch, key_off, sources, who, 500, nd, ("pairs", nd))
        assert cuts == [600 * s // nd for s in range(nd + 1)]
    # the keys of slice 0 (of 3) all held inside block 0 (KSP_REORDER=0: block = source // 128)
    counts = [3 + k % 4 for k in range(90)]
    cuts = S.postings_cuts(np.concatenate([[0], np.cumsum(counts)]), 3)
    key_off, sources, who = _postings_input(counts, 400, seed=4, same_block=set(range(cuts[1])))
    assert max(max(who[k]) for k in range(cuts[1])) < 128 <= max(max(who[k]) for k in range(cuts[1], 90))
    _check_postings(monkeypatch, key_off, sources, who, 400, 3, "one block", env={"KSP_REORDER": "0"})
    _check_postings(monkeypatch, key_off, sources, who, 400, 3, "one block, default order")


@pytest.mark.parametrize("total", [65535, 65536, 65537, 80000])
def test_postings_slices_whose_bounds_pass_16_bits_only_together(monkeypatch, total):
    """Sources 0 and 128 (two blocks) hold the same 4 keys, a key per slice: weighted, the weights sum to `total` (no
    slice sees more than a quarter); unweighted, `total` keys of two holders in 3 slices.  The counter width of the
    assembled lists must come from the sums over the slices, not from one slice's share."""
    key_off = np.arange(5, dtype=np.uint64) * 2
    sources = np.array([0, 128] * 4, dtype=np.uint32)
    wts = np.array([total // 4] * 3 + [total - 3 * (total // 4)], dtype=np.uint32)
    want = S.edges_of({(0, 128): total})
    for env in ({"KSP_REORDER": "0"}, {}, {"KSP_REORDER": "0", "KSP_NO_SCHED": "1"}, {"KSP_JOIN": "window"}):
        _env(monkeypatch, dict(env, KSP_SLICES=4))
        edges, st = engine.pairwise_postings_host(key_off, sources, wts, 129)
        _same(edges, want, (total, env, "KSP_SLICES"))
        assert st["weighted"]
        _env(monkeypatch, env)
        edges, _ = engine.pairwise_postings_host(key_off, sources, wts, 129, devices=[0] * 4)
        _same(edges, want, (total, env, "devices"))
        edges, sizes, _ = sliced_postings_edges(key_off, sources, wts, 129, [0, 1, 2, 3, 4])
        _same(edges, want, (total, env, "driver"))
        assert sizes[1::4].tolist() == [1, 1, 1, 1]
        # a caller that leaves the bounds exchange out: 32-bit counters everywhere, the same edges
        edges, _, _ = sliced_postings_edges(key_off, sources, wts, 129, [0, 1, 2, 3, 4], sum_bounds=False)
        _same(edges, want, (total, env, "driver without the bounds exchange"))
    key_off = np.arange(total + 1, dtype=np.uint64) * 2
    sources = np.tile(np.array([0, 128], dtype=np.uint32), total)
    cuts = S.postings_cuts(key_off, 3)
    assert max(b - a for a, b in zip(cuts, cuts[1:])) < 65535
    for env in ({"KSP_REORDER": "0"}, {}, {"KSP_REORDER": "0", "KSP_JOIN": "matches"}, {"KSP_REORDER": "0", "KSP_JOIN": "window"}):
        _env(monkeypatch, dict(env, KSP_SLICES=3))
        edges, _ = engine.pairwise_postings_host(key_off, sources, None, 129)
        _same(edges, want, (total, env, "unweighted, KSP_SLICES"))
        _env(monkeypatch, env)
        edges, sizes, _ = sliced_postings_edges(key_off, sources, None, 129, cuts)
        _same(edges, want, (total, env, "unweighted, driver"))
        edges, _, _ = sliced_postings_edges(key_off, sources, None, 129, cuts, sum_bounds=False)
        _same(edges, want, (total, env, "unweighted, driver without the bounds exchange"))
        assert sizes[1::4].tolist() == [b - a for a, b in zip(cuts, cuts[1:])]


# ---- E. one full-size run ----------------------------------------------------------------------------------------------
def test_c3_full_size_in_three_slices(monkeypatch):
    """C3 (100 000 sources, ~780 blocks), the config the multi-GPU design is meant for, assembled from 3 slices: the
    whole edge set by pair_probe.check_edge_set as in test_large_gpu.py, and row for row the unsliced run."""
    sk, idx = config("C3")
    assert sk.n_sources == 100_000
    one, st1 = engine.pairwise_host(sk.keys, sk.offsets)
    monkeypatch.setenv("KSP_SLICES", "3")
    ev, st = engine.pairwise_host(sk.keys, sk.offsets)
    monkeypatch.delenv("KSP_SLICES")
    assert st["n_entries"] == int(sk.offsets[-1]) and st["n_blocks"] > 256 and len(ev) > 100_000
    assert st["n_kept_keys"] == st1["n_kept_keys"]
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=11)
    assert len(ev) == len(one) and (ev == one).all()

"""The session of classify on the device (csrc/classify.hip: ksp_classify_open / _add / _finish / _close): one batch against
many batches with a record cut so that a hit hash lies in both pieces, the hit buffer's compaction and regrowth with the counts
a model of the rule predicts, finish without add, close without finish, and refused calls that leave the session usable."""
import random

import pytest

import classify_inputs as CI
import classify_restate as CR
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu

K = 21
FULL = CI.FULL
same = CI.check_result


@pytest.fixture(scope="module")
def world():
    """Four records: 0 = A + X + B + X + C with a k-mer X (cut inside the second X below); 1 = D, a break byte, D again: every hit
    word twice; 2 random; 3 shorter than k.  The references of classify_inputs and one that holds X's hash alone."""
    rng = random.Random(91)
    x, d = I.bases(rng, K), I.bases(rng, 300)
    recs = [I.bases(rng, 700) + x + I.bases(rng, 700) + x + I.bases(rng, 200), d + "N" + d, I.bases(rng, 400, lower=0.3), I.bases(rng, K - 1)]
    seq = "".join(r + "\n" for r in recs).encode()
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r) + 1)
    kept = CR.record_hashes(seq, off, K, FULL)
    x_hash = R.kmer_hash(x)
    refs = CI.references(kept) + [[x_hash]]
    cut = 700 + K + 700 + 10   # inside the second X: that window lies in the second piece, the first X in the first
    pieces = [  # (bytes, segment offsets, segment records) of three batches
        (recs[0][:cut].encode(), [0, cut], [0]),
        ((recs[0][cut - (K - 1):] + "\n" + recs[1] + "\n").encode(), [0, len(recs[0]) - cut + K, len(recs[0]) - cut + K + len(recs[1]) + 1], [0, 1]),
        ((recs[2] + "\n" + recs[3] + "\n").encode(), [0, len(recs[2]) + 1, len(recs[2]) + len(recs[3]) + 2], [2, 3]),
    ]
    return {"seq": seq, "off": off, "kept": kept, "refs": refs, "flat": CR.flat_refs(refs), "want": CR.from_kept(kept, refs), "pieces": pieces, "x_hash": x_hash, "recs": recs}


def _words(world, piece):
    """The hit words a batch appends, as (record, hash) with repeats."""
    data, off, rec = piece
    everything = {h for q in world["refs"] for h in q}
    return [(rec[s], h) for s, run in enumerate(CR.record_hashes(data, off, K, FULL)) for h in run if h in everything]


def _model(first, batches):
    """(retries, compactions) the rule of the hit buffer gives for batches of hit words and a first capacity."""
    cap, held, retries, compactions = first, [], 0, 0
    for words in batches:
        if len(words) > cap - len(held):
            if held:
                held = sorted(set(held))
                compactions += 1
            if len(words) > cap - len(held):
                cap = len(held) + len(words)
            retries += 1
        held = held + words
    return retries, compactions


def _session(world, pieces, n_records=4, min_hits=1):
    ref_keys, ref_off = world["flat"]
    with engine.ClassifySession(K, ref_keys, ref_off, max_hash=FULL) as s:
        for data, off, rec in pieces:
            s.add(data, off, rec)
        return s.finish(n_records, min_hits)


def test_one_batch_equals_many_with_a_record_cut_across_them(world):
    one = _session(world, [(world["seq"], world["off"], [0, 1, 2, 3])])
    st_one = same(one, world["want"], "one batch")
    many = _session(world, world["pieces"])
    st_many = same(many, world["want"], "three batches")
    assert (one[0] == many[0]).all() and all((one[1][name] == many[1][name]).all() for name in one[1])
    assert st_one["batches"] == 1 and st_many["batches"] == 3 and st_one["hit_words"] == st_many["hit_words"]   # every window lies in one piece
    # X's hash is a hit in both pieces of record 0 and counts once
    assert any(h == world["x_hash"] for _, h in _words(world, world["pieces"][0])) and any(r == 0 and h == world["x_hash"] for r, h in _words(world, world["pieces"][1]))
    assert (0, len(world["refs"]) - 1, 1) in world["want"]["rows"]
    assert world["kept"][0].count(world["x_hash"]) == 2 and world["want"]["kept_windows"][0] > len(set(world["kept"][0]))


def test_compaction_and_regrowth_follow_the_rule(world, monkeypatch):
    """Batches in an order that holds duplicate words (record 1 says everything twice): a first capacity that the compaction
    alone rescues, one that needs the regrowth as well, 1, and the exact need."""
    recs = world["recs"]
    pieces = [((recs[1] + "\n").encode(), [0, len(recs[1]) + 1], [1]), world["pieces"][2], world["pieces"][0], ((recs[0][700 + K + 700 + 10 - (K - 1):] + "\n").encode(),
                                                                                                               [0, len(recs[0]) - (700 + K + 700 + 10) + K], [0])]
    batches = [_words(world, p) for p in pieces]
    n = [len(b) for b in batches]
    assert n[0] == 2 * len(set(batches[0])) > 0 and min(n) > 0
    rescued = n[0] + n[1] - 1
    assert _model(rescued, batches[:2]) == (1, 1)
    seen = set()
    for first in (rescued, 1, n[0], sum(n) - 1, sum(n)):
        want = _model(first, batches)
        seen.add(want)
        monkeypatch.setenv("KSPIDER_CLASSIFY_FIRST_CAPACITY", str(first))
        st = same(_session(world, pieces), world["want"], first)
        assert (st["retries"], st["compactions"]) == want, first
        assert st["hit_words"] == sum(n) and st["batches"] == 4
    assert (0, 0) in seen and any(c for _, c in seen) and any(r > c for r, c in seen)


def test_finish_without_add_and_close_without_finish(world):
    rows, arrays, st = _session(world, [], n_records=3)
    assert rows.size == 0 and st["batches"] == 0 and st["table_keys"] > 0
    assert all(not arrays[name].any() for name in arrays if name != "best_ref") and (arrays["best_ref"] == engine.CLASSIFY_NO_REF).all()
    ref_keys, ref_off = world["flat"]
    s = engine.ClassifySession(K, ref_keys, ref_off, max_hash=FULL)
    s.add(world["seq"], world["off"], [0, 1, 2, 3])
    s.close()
    s.close()   # (the wrapper forgets the handle: the library sees one close)
    engine.lib().ksp_classify_close(None)


def test_refused_calls_leave_the_session_usable(world):
    ref_keys, ref_off = world["flat"]

    def refuse(call, *args):
        with pytest.raises(engine.KspError) as ei:
            call(*args)
        assert ei.value.code == engine.KSP_E_ARG, str(ei.value)

    with engine.ClassifySession(K, ref_keys, ref_off, max_hash=FULL) as s:
        data, off, rec = world["pieces"][0]
        refuse(s.add, data, [0, len(data) - 1], rec)            # the offsets do not end at n_bytes
        refuse(s.add, data, [1, len(data)], rec)
        refuse(s.add, data, off, [0xFFFFFFFF])
        refuse(s.add, data, off, None)
        refuse(s.add, data, [0], [])
        for piece in world["pieces"]:
            s.add(*piece)
        refuse(s.finish, 3)                                     # record 3 was added
        refuse(s.finish, 4, 0)                                  # min_hits = 0
        same(s.finish(4), world["want"], "after refusals")
        refuse(s.add, data, off, rec)                           # the session is finished
        refuse(s.finish, 4)
    with pytest.raises(engine.KspError) as ei:
        engine.ClassifySession(K, ref_keys, ref_off, max_hash=FULL, device=99)
    assert ei.value.code == engine.KSP_E_HIP and "no such device" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.ClassifySession(K, [2, 1], [0, 2], max_hash=FULL)
    assert ei.value.code == engine.KSP_E_ARG


def test_more_records_than_were_added(world):
    """n_records above every id: the records that no batch named are empty rows of the arrays."""
    rows, arrays, _ = _session(world, world["pieces"], n_records=7)
    assert [tuple(int(v) for v in (x["record"], x["reference"], x["hits"])) for x in rows] == world["want"]["rows"]
    assert arrays["kept_windows"].tolist() == world["want"]["kept_windows"] + [0, 0, 0] and arrays["best_ref"][4:].tolist() == [CR.NO_REF] * 3

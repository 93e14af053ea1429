"""Seeded inputs of the classify tests (CPU and GPU).  The records come from tests/sketch_inputs.py (every Case's sources are the
records) and from repeats() below; the references are derived from the restated kept hashes of the records themselves, so that
every edge the definition names occurs: tests/test_classify_inputs_cpu.py checks that it does."""
import functools
import gzip
import json
import random

import classify_restate as CR
import sketch_inputs as I
import sketch_restate as R

FULL = 2**64 - 1

# the references of references(): their order is part of the cases
HALF, THIRD, EMPTY, NOWHERE, COPY, PAIR = range(6)
REF_NAMES = ["half", "third", "empty", "nowhere", "copy_of_half", "pair"]


def repeats(k, seed=21):
    """Four records, each followed by a newline:
       0  a random sequence, a break byte, and its first k + 5 bases again: six k-mers occur twice, kept_windows > |S|;
       1  a random sequence, a break byte, and the reverse complement of its first k + 5 bases: the same, by the other strand;
       2  fewer than k bases (k = 1: only a break byte);
       3  the `lonely` record: a random sequence whose hashes references() keeps out of every reference."""
    rng = random.Random(seed * 1000 + k)
    a, b, lonely = I.bases(rng, 60 + k, lower=0.2), I.bases(rng, 60 + k), I.bases(rng, 50 + k)
    recs = [a + "N" + a[:k + 5], b + "N" + R.revcomp(b[:k + 5]), I.bases(rng, k - 1) if k > 1 else "N", lonely]
    seq = "".join(r + "\n" for r in recs).encode()
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r) + 1)
    return I.Case("repeats", seq, off)


LONELY = 3   # the record of repeats() that hits nothing


def references(kept, lonely=None, seed=22):
    """Six references from the kept hashes of the records (CR.record_hashes), without those of record `lonely`:
       HALF every 2nd hash of the union; THIRD every 3rd; EMPTY none; NOWHERE hashes that occur in no record; COPY the same as
       HALF (the tie for best); PAIR the union's first hash — which HALF, THIRD and COPY hold too: four holders — and its middle one."""
    away = set(kept[lonely]) if lonely is not None else set()
    union = sorted({h for r, run in enumerate(kept) if r != lonely for h in run} - away)
    rng = random.Random(seed)
    everything = set(union) | away
    nowhere = set()
    while len(nowhere) < 40:
        h = rng.getrandbits(64)
        if h not in everything:
            nowhere.add(h)
    pair = sorted({union[0], union[len(union) // 2]}) if union else []
    return [union[::2], union[::3], [], sorted(nowhere), union[::2], pair]


@functools.lru_cache(maxsize=None)
def restated(case_key, k, max_hash=FULL):
    """(case, kept hashes per record, references, flat references) of a named case, made once: case_key = (generator name, index)."""
    name, index = case_key
    made = {"repeats": lambda: [repeats(k)], "mixed": lambda: [I.mixed()], "junction": lambda: [I.junction(k)], "boundaries": lambda: I.boundaries(k),
            "tile_edges": lambda: I.tile_edges(k), "reads": lambda: [I.short_reads()[1]]}[name]()
    case = made[index]
    kept = CR.record_hashes(case.seq, case.offsets, k, max_hash)
    refs = references(kept, LONELY if name == "repeats" else None)
    return case, kept, refs, CR.flat_refs(refs)


def small_keys(k):
    """The cases every ksize takes part in on the CPU: a few thousand bytes each."""
    return [("repeats", 0), ("mixed", 0), ("junction", 0)] + [("boundaries", i) for i in range(3)]


def edge_keys(k):
    """The tile-edge cases of tests/sketch_inputs.py: one record of T - 1, T, T + 1, T + k - 1 and 2T + 1 bases, without and with a
    break byte at T - 1, T and T + k - 2."""
    return [("tile_edges", i) for i in range(len(I.tile_edges(k)))]


def middle_hits(rows):
    """A min_hits M with rows below it and rows at or above it: the median of the distinct hit counts above the smallest."""
    values = sorted({n for _, _, n in rows})
    assert len(values) >= 2, "the rows have one hit count only"
    return values[max(1, len(values) // 2)]


def check_result(got, want, what):
    """(rows, arrays, stats) of an engine.classify_* call against a result of the restatement; returns the stats."""
    rows, arrays, st = got
    assert [tuple(int(v) for v in (x["record"], x["reference"], x["hits"])) for x in rows] == want["rows"], what
    assert not rows["reserved"].any()
    for name in ("kept_windows", "matched", "n_refs_hit", "best_ref", "best_hits", "second_hits"):
        assert arrays[name].tolist() == want[name], (what, name)
    assert st["rows"] == len(want["rows"]) and st["kept_windows"] == sum(want["kept_windows"]) and st["hit_words_unique"] == sum(want["matched"]), what
    return st


def hit_words(kept, refs):
    """What a batch of these records appends: one word per kept window whose hash a reference holds."""
    everything = {h for q in refs for h in q}
    return sum(1 for run in kept for h in run if h in everything)


# ---- the files of the driver tests (CPU: host mode against the restatement; GPU: device mode against host mode)
FILES_K, FILES_SCALED = 21, 2
FILES_MH = R.max_hash_of(FILES_SCALED)
# the database's groups in glob order; "3_other_k" has no signature of ksize FILES_K: it keeps its id and is never hit
GROUPS = ["1_half", "2_third", "3_other_k", "4_empty", "5_nowhere", "6_copy", "7_pair"]
REF_IDS = [1, 2, 4, 5, 6, 7]
FILE_REF_NAMES = [GROUPS[i - 1] for i in REF_IDS]


def _fasta(records, width=60):
    return "".join(">" + name + "\n" + "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width)) for name, seq in records)


def _fastq(records):
    return "".join("@" + name + "\n" + seq + "\n+\n" + "I" * len(seq) + "\n" for name, seq in records)


def _make_records():
    """(records of the first file, of the second).  The first record is A + X + B + X + C with a k-mer X: `CUT` bytes of batch
    end in the middle of the second X, so that X's hash lies in both pieces of the record."""
    rng = random.Random(77)
    x = I.bases(rng, FILES_K)
    long_one = I.bases(rng, 700) + x + I.bases(rng, 700, lower=0.2) + x + I.bases(rng, 200)
    first = [("contig/1 len=" + str(len(long_one)), long_one)]
    for i in range(12):
        s = list(I.bases(rng, rng.randint(30, 300), lower=0.2))
        s[rng.randrange(len(s))] = "N"
        first.append((f"read{i % 5}", "".join(s)))   # names repeat
    first.append(("short", I.bases(rng, FILES_K - 1)))
    first.append(("empty", ""))
    second = [(f"read{i}", I.bases(rng, rng.randint(60, 200))) for i in range(8)]
    return first, second


CUT = 700 + FILES_K + 700 + FILES_K // 2


def files_world(d):
    """Reads (a directory: a.fa, b.fq.gz), a database directory of .sig files and everything the restatement says about them, under the directory d."""
    first, second = _make_records()
    reads = d / "reads"
    reads.mkdir()
    (reads / "a.fa").write_text(_fasta(first))
    (reads / "b.fq.gz").write_bytes(gzip.compress(_fastq(second).encode()))
    (reads / "ignored.txt").write_text("not a sequence file\n")
    records = first + second
    seq = "".join(s + "\n" for _, s in records).encode()
    off = [0]
    for _, s in records:
        off.append(off[-1] + len(s) + 1)
    names = [n.split()[0] for n, _ in records]
    lengths = [len(s) for _, s in records]
    refs = references(CR.record_hashes(seq, off, FILES_K, FULL))   # from ALL hashes: about half of a reference lies above FILES_MH
    db = d / "db"
    db.mkdir()
    for group, q in zip(FILE_REF_NAMES, refs):
        sig = [{"class": "sourmash_signature", "filename": group, "signatures": [{"num": 0, "ksize": FILES_K, "seed": 42, "max_hash": 0, "molecule": "DNA", "mins": [int(h) for h in q]}]}]
        (db / (group + ".sig")).write_text(json.dumps(sig))
    other = [{"class": "sourmash_signature", "filename": "x", "signatures": [{"num": 0, "ksize": 31, "seed": 42, "max_hash": 0, "molecule": "DNA", "mins": [1, 2, 3]}]}]
    (db / "3_other_k.sig").write_text(json.dumps(other))
    kept = CR.record_hashes(seq, off, FILES_K, FILES_MH)
    return {"dir": d, "reads": reads, "db": db, "seq": seq, "off": off, "names": names, "lengths": lengths, "refs": refs, "kept": kept, "n_first": len(first)}

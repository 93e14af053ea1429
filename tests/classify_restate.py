"""The definition of classify (include/kspider_amd.h, "classify") in plain Python, on top of the restated sketch arithmetic of
tests/sketch_restate.py: per record the kept hashes as a list (windows) and as a set, intersections with every reference as
Python sets, the cut at min_hits, the summary by sorting.  Nothing here shares code with the library."""
import sketch_restate as R

NO_REF = 0xFFFFFFFF


def record_hashes(seq: bytes, rec_offsets, ksize: int, max_hash: int, seed: int = 42) -> list:
    """Per record the kept hashes of its windows, in order of position (with repeats)."""
    out = []
    for r in range(len(rec_offsets) - 1):
        text = bytes(seq[int(rec_offsets[r]):int(rec_offsets[r + 1])])
        out.append([h for h in R.source_hashes(text, ksize, seed) if h <= max_hash])
    return out


def from_kept(kept: list, refs, min_hits: int = 1) -> dict:
    """The result for records whose kept hashes (with repeats) are given: rows [(record, reference, hits)] ordered by (record,
    reference), and the six per-record lists."""
    ref_sets = [set(int(h) for h in q) for q in refs]
    everything = set().union(*ref_sets) if ref_sets else set()
    out = {"rows": [], "kept_windows": [], "matched": [], "n_refs_hit": [], "best_ref": [], "best_hits": [], "second_hits": []}
    for r, windows in enumerate(kept):
        S = set(windows)
        mine = [(q, len(S & ref_sets[q])) for q in range(len(ref_sets))]
        mine = [(q, n) for q, n in mine if n >= min_hits and n > 0]
        out["rows"] += [(r, q, n) for q, n in mine]
        out["kept_windows"].append(len(windows))
        out["matched"].append(len(S & everything))
        out["n_refs_hit"].append(len(mine))
        ranked = sorted(mine, key=lambda x: (-x[1], x[0]))   # the largest first, a tie to the smaller reference
        out["best_ref"].append(ranked[0][0] if ranked else NO_REF)
        out["best_hits"].append(ranked[0][1] if ranked else 0)
        out["second_hits"].append(ranked[1][1] if len(ranked) > 1 else 0)
    return out


def classify(seq: bytes, rec_offsets, ksize: int, max_hash: int, refs, min_hits: int = 1, seed: int = 42) -> dict:
    return from_kept(record_hashes(seq, rec_offsets, ksize, max_hash, seed), refs, min_hits)


def flat_refs(refs) -> tuple:
    """(keys, offsets) of the references as the library takes them: every run ascending."""
    return R.flat([sorted(int(h) for h in q) for q in refs])


def summary_tsv(names, lengths, res: dict, ref_names) -> str:
    """OUT_kSpider_classify.tsv for records named `names` with sequences of `lengths` bytes."""
    lines = ["record_id\tname\tlength\tkept_windows\tmatched\tn_refs\tbest_ref\tbest_hits\tsecond_hits\n"]
    for r, name in enumerate(names):
        best = res["best_ref"][r]
        lines.append("\t".join(str(x) for x in (r + 1, name, lengths[r], res["kept_windows"][r], res["matched"][r], res["n_refs_hit"][r],
                                                 "-" if best == NO_REF else ref_names[best], res["best_hits"][r], res["second_hits"][r])) + "\n")
    return "".join(lines)


def hits_tsv(names, res: dict, ref_names, ref_ids=None) -> str:
    """OUT_kSpider_classify_hits.tsv; ref_ids: the database id of every reference (its position + 1 when not given)."""
    lines = ["record_id\tname\tref_id\tref_name\thits\n"]
    for r, q, n in res["rows"]:
        lines.append("\t".join(str(x) for x in (r + 1, names[r], ref_ids[q] if ref_ids else q + 1, ref_names[q], n)) + "\n")
    return "".join(lines)

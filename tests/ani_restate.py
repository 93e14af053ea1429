"""Python restatement of `kSpider pairwise --estimate-ani` (pykSpider/kSpider2/ks_pairwise.py:29-84) for the tests.

sourmash is not installed, so containment_to_distance's point estimate and ANIResult.ani are restated from their
documented behaviour rather than called: no reference-generated output pins these values."""
import numpy as np


def g(text, k):
    """ANIResult.ani of containment_to_distance(float(text), k, ...): 1 - point estimate of the distance."""
    c = float(text)
    if c != c:
        raise ValueError("NaN containment")   # sourmash rejects it
    if c <= 0.0001:
        pe = 1.0
    elif c >= 0.9999:
        pe = 0.0
    else:
        pe = 1.0 - c ** (1.0 / k)
    return 1 - pe


def ani_text(t3, t5, k):
    """The line ks_pairwise.py writes for a row with column texts t3 (min) and t5 (max)."""
    return f"{(g(t3, k) + g(t5, k)) / 2.0}"


def float_text(v):
    """Text of an f32 as the pairwise writer prints it (std::ostream << float: '%.6g' of the float as a double)."""
    return "%.6g" % float(np.float32(v))


def ani_of_floats(mn, mx, k):
    return (g(float_text(mn), k) + g(float_text(mx), k)) / 2.0


def estimate_ani(prefix, scale):
    """The bytes of PREFIX_kSpider_pairwise.ani_col.tsv as ks_pairwise.py writes them; raises where it would fail."""
    if not scale:
        raise ValueError("estimating ANI requires to provide --scale value")
    with open(f"{prefix}.extra") as extra:
        k = int(next(extra))
    kmers = {}
    with open(f"{prefix}_kSpider_seqToKmersNo.tsv") as f:
        next(f)
        for line in f:
            seq_id, n = tuple(line.strip().split("\t")[1:])
            kmers[int(seq_id)] = int(n)
    out = ["avg_ani\n"]
    with open(f"{prefix}_kSpider_pairwise.tsv") as f:
        next(f)
        for or_line in f:
            line = or_line.strip().split("\t")
            int(line[2])
            id_1, id_2 = int(line[0]), int(line[1])
            kmers[id_2], kmers[id_1]   # KeyError for an unknown id
            out.append(ani_text(line[3], line[5], k) + "\n")
    return "".join(out).encode()

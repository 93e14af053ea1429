"""The containment cut restated (tests only): a row is kept exactly when `kSpider cluster` keeps it for that column and
cut-off (ks_clustering.py:101-105) — text -> Python float -> x 100 -> not below cutoff x 100; a NaN is not below anything.
Nothing here calls the code under test; a float becomes text through engine.format_float, which existing tests pin."""
import numpy as np

from kspider_amd import engine
from repr_restate import column_values   # the float maths of src/pairwise.cpp:260-264 in numpy.float32


def keep(text: str, cutoff: float) -> bool:
    return not (float(text) * 100 < cutoff * 100)


def cut_tsv(tsv_text: str, col: int, cutoff: float) -> str:
    lines = tsv_text.split("\n")
    return "\n".join(lines[:1] + [l for l in lines[1:] if not l or keep(l.split("\t")[col], cutoff)])


def edge_mask(edges: np.ndarray, kmer_counts: np.ndarray, col: int, cutoff: float) -> np.ndarray:
    """Per edge, through the text of its own column value."""
    vals = column_values(edges, np.asarray(kmer_counts), col)
    return np.array([keep(engine.format_float(v), cutoff) for v in vals.tolist()], dtype=bool)

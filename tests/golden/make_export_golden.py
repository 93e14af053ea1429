#!/usr/bin/env python3
"""Golden vectors for `kSpider export`: the REFERENCE's own command
(pykSpider/kSpider2/ks_export.py, loaded from where it lies, unmodified, with a stub `_kSpider_internal`) is run
on the pairwise TSVs of the two committed signature sets (tests/golden/clusters/) and on small hand-written inputs
that hit every quirk of its pandas / scipy path.  Stored under tests/golden/export/<case>/: the inputs it read and
the files it wrote (ref_<dist>_pairwise.tsv, ref_<dist>_distmat.tsv, ref_<dist>.newick).  Nothing of the
reference is copied.

Run from the repo root (needs the reference checkout, click, pandas, scipy):
    python tests/golden/make_export_golden.py [REFERENCE_ROOT]"""
import importlib.util
import os
import shutil
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
REF_PKG = os.path.join(REF_ROOT, "pykSpider", "kSpider2")

import ani_restate  # noqa: E402

DISTS = ("min_cont", "avg_cont", "max_cont", "ani")
HEADER = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n"

# hand-written inputs: names (id order), rows (id1, id2, min, avg, max); shared k-mers and k-mer counts are unused
QUIRKS = {
    # a NaN row, containments 0 and 1, exponent texts both ways, an all-NaN column (node e), a name with '"',
    # equal distances
    "quirks": (["n1", 'b"x', "c", "d", "e", "f", "zz", "Ab"],
               [(1, 2, "0.5", "0.6", "0.7"), (1, 3, "0", "0", "0"), (2, 3, "1", "1", "1"),
                (3, 4, "1e-05", "2e-05", "3e-05"), (4, 5, "nan", "nan", "nan"), (5, 6, "nan", "nan", "nan"),
                (6, 7, "0.0117647", "0.0117647", "0.0117647"), (1, 7, "0.0117647", "0.0117647", "0.0117647"),
                (7, 8, "0.999999", "0.9999995", "0.9999999"), (2, 8, "1e-23", "0.00015", "0.25")]),
    # duplicate sources: every distance equal, then two groups of identical rows — Prim's ties decide the tree
    "ties": (["s5", "s1", "s4", "s2", "s3", "s6"],
             [(a, b, "0.5", "0.5", "0.5") for a in range(1, 7) for b in range(a + 1, 7) if (a <= 3) == (b <= 3)]
             + [(a, b, "0.25", "0.25", "0.25") for a in range(1, 4) for b in range(4, 7)]),
    "two": (["left", "right"], [(1, 2, "0.3", "0.4", "0.5")]),
}


def load_reference_export():
    """ks_export.py imports `_kSpider_internal` (unused by export) and `from kSpider2.click_context import cli`; the
    package's __init__ would drag in the SWIG extension, so the modules it needs are loaded by path."""
    os.environ.pop("BRANCH_NAME", None)      # with it set, kSpider_version.get_version asks test.pypi.org
    sys.modules["_kSpider_internal"] = types.ModuleType("_kSpider_internal")
    pkg = types.ModuleType("kSpider2")
    pkg.__path__ = [REF_PKG]
    sys.modules["kSpider2"] = pkg
    for name in ("customLogger", "kSpider_version", "click_context", "ks_export"):
        spec = importlib.util.spec_from_file_location("kSpider2." + name, os.path.join(REF_PKG, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["kSpider2." + name] = mod
        spec.loader.exec_module(mod)
    return sys.modules["kSpider2.ks_export"].main, sys.modules["kSpider2.customLogger"].Logger


def write_inputs(d, names, rows):
    prefix = os.path.join(d, "sigs")
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {nm}\n" for i, nm in enumerate(names)))
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n" + "".join(f"{i + 1}\t{i + 1}\t100\n" for i in range(len(names))))
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write(HEADER + "".join(f"{a}\t{b}\t1\t{mn}\t{av}\t{mx}\n" for a, b, mn, av, mx in rows))
    return prefix


def main():
    export, Logger = load_reference_export()
    sys.setrecursionlimit(100000)
    out_root = os.path.join(HERE, "export")
    shutil.rmtree(out_root, ignore_errors=True)
    cases = {}
    for tag in ("setA", "setB"):
        d = os.path.join(out_root, tag)
        os.makedirs(d)
        src = os.path.join(HERE, "clusters", tag, "sigs")
        for suf in (".namesMap", "_kSpider_seqToKmersNo.tsv", "_kSpider_pairwise.tsv"):
            shutil.copy(src + suf, os.path.join(d, "sigs" + suf))
        prefix = os.path.join(d, "sigs")
        with open(prefix + ".extra", "w") as f:       # k = 21; estimate_ani only reads the first line
            f.write("21\n")
        with open(prefix + "_kSpider_pairwise.ani_col.tsv", "wb") as f:
            f.write(ani_restate.estimate_ani(prefix, 1000))
        os.remove(prefix + ".extra")
        cases[tag] = (prefix, DISTS)
    for tag, (names, rows) in QUIRKS.items():
        d = os.path.join(out_root, tag)
        os.makedirs(d)
        cases[tag] = (write_inputs(d, names, rows), DISTS[:3])
    for tag, (prefix, dists) in cases.items():
        for dist in dists:
            out = os.path.join(os.path.dirname(prefix), f"ref_{dist}")
            export.main(args=["-i", prefix, "-d", dist, "--newick", "-o", out], obj=Logger(False), standalone_mode=False)
            for suf in ("_pairwise.tsv", "_distmat.tsv", ".newick"):
                assert os.path.exists(out + suf), out + suf
            print(tag, dist, "->", os.path.basename(out), os.path.getsize(out + "_distmat.tsv"), "bytes of matrix")


if __name__ == "__main__":
    main()

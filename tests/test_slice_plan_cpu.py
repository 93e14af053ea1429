"""The slice plan of a multi-device job (kspider_amd/csrc/slice_plan.h: how many slices, the device of each, the keys of every
postings slice) on the CPU, through the `plan` subcommand of the sanitizer build (`make -C kspider_amd/csrc asan`): against the
restatement tests/slice_inputs.postings_cuts on the shapes tests/test_slices_edges_gpu.py section D runs on the GPU, and
against values worked out here for what no GPU test builds: 2^30 entries or more, the limits, more slices than keys."""
import pytest

import slice_inputs as S
from test_host_hardening_cpu import _run, exe   # noqa: F401  (exe: the fixture that builds the program)

KSP_E_LIMIT = 5
TOO_LARGE = "pairwise: one colour range holds 2^30 memberships or more (a single colour that large?)"


def _plan(exe, monkeypatch, *args, slices=None):
    """(rc, message) of a refused plan, else (0, {"devices": [...], "cuts": [...], "sliced": bool})."""
    if slices is None:
        monkeypatch.delenv("KSP_SLICES", raising=False)
    else:
        monkeypatch.setenv("KSP_SLICES", str(slices))
    rc, line, out = _run(exe, "plan", *[str(a) for a in args])
    if rc:
        return rc, line.split(None, 2)[2]
    rows = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines() if not l.startswith("rc ")}
    assert rows["slices"] == [len(rows["devices"])], out
    return 0, {"devices": rows["devices"], "cuts": rows["cuts"], "sliced": bool(rows["sliced"][0])}


def _postings(exe, monkeypatch, counts, devices, slices=None):
    return _plan(exe, monkeypatch, "postings", ",".join(str(d) for d in devices), *counts, slices=slices)


def _sketch(exe, monkeypatch, n, devices, slices=None):
    return _plan(exe, monkeypatch, "sketch", n, ",".join(str(d) for d in devices), slices=slices)


def _half_shape(at):
    small = [2 + k % 3 for k in range(120)]
    return small[:at] + [sum(small)] + small[at:]


SHAPES = {   # (what tests/test_slices_edges_gpu.py section D builds)
    "keys nd-1": lambda nd: [2 + (3 * k) % 5 for k in range(nd - 1)],
    "keys nd": lambda nd: [2 + (3 * k) % 5 for k in range(nd)],
    "keys nd+1": lambda nd: [2 + (3 * k) % 5 for k in range(nd + 1)],
    "half first": lambda nd: _half_shape(0),
    "half middle": lambda nd: _half_shape(60),
    "half last": lambda nd: _half_shape(120),
    "600 of 2": lambda nd: [2] * 600,
}


@pytest.mark.parametrize("nd", [2, 3, 5, 7])
def test_postings_cuts_are_the_restatement(exe, monkeypatch, nd):
    """nd devices, and one device with KSP_SLICES=nd: the cuts of slice_inputs.postings_cuts, one slice per device (taken round
    robin); fewer keys than slices is one whole build on every device of the job, no cuts."""
    for what, shape in SHAPES.items():
        counts = shape(nd)
        key_off = [0]
        for c in counts:
            key_off.append(key_off[-1] + c)
        want = S.postings_cuts(key_off, nd)
        whole = want == [0, len(counts)]
        assert whole == (len(counts) < nd), (what, nd, want)
        rc, many = _postings(exe, monkeypatch, counts, [0] * nd)
        assert rc == 0 and many == {"devices": [0] * nd, "cuts": [] if whole else want, "sliced": not whole}, (what, nd, many, want)
        rc, forced = _postings(exe, monkeypatch, counts, [3], slices=nd)
        assert rc == 0 and forced == {"devices": [3] * (1 if whole else nd), "cuts": [] if whole else want, "sliced": not whole}, (what, nd, forced, want)


def test_an_index_without_keys_is_one_whole_build_on_every_device(exe, monkeypatch):
    """0 keys (the entry points take a NULL key_off then, and so does the program): more slices than keys below 2^30, so no
    cuts and nothing sliced, on one device or several and whatever KSP_SLICES asks for."""
    for devices, slices in (([0], None), ([0, 0], None), ([1, 2, 1], None), ([0], 3), ([0, 0], 5)):
        assert _postings(exe, monkeypatch, [], devices, slices=slices) == (0, {"devices": devices, "cuts": [], "sliced": False}), (devices, slices)


def test_sketch_slices_by_entry_count_devices_and_env(exe, monkeypatch):
    """Below 2^30 entries one build per device of the job; from 2^30 on n // 900 000 000 + 1 slices (2^30 // 9e8 = 1: two);
    more slices than devices take the devices round robin; 65 slices (64 * 9e8 entries) are refused."""
    assert _sketch(exe, monkeypatch, 2**30 - 1, [4]) == (0, {"devices": [4], "cuts": [], "sliced": False})
    assert _sketch(exe, monkeypatch, 2**30, [4]) == (0, {"devices": [4, 4], "cuts": [], "sliced": True})
    assert _sketch(exe, monkeypatch, 1000, [7], slices=3) == (0, {"devices": [7, 7, 7], "cuts": [], "sliced": True})
    assert _sketch(exe, monkeypatch, 1000, [2, 5], slices=5) == (0, {"devices": [2, 5, 2, 5, 2], "cuts": [], "sliced": True})
    assert _sketch(exe, monkeypatch, 1000, [2, 5, 2], slices=2) == (0, {"devices": [2, 5, 2], "cuts": [], "sliced": True})   # (never fewer than the devices)
    assert _sketch(exe, monkeypatch, 0, [1], slices=0) == (0, {"devices": [1], "cuts": [], "sliced": False})
    assert _sketch(exe, monkeypatch, 64 * 900_000_000, [0]) == (KSP_E_LIMIT, "pairwise_host: more than 2^35 key entries")
    assert _sketch(exe, monkeypatch, 64 * 900_000_000 - 1, [0, 1])[1]["devices"] == [0, 1] * 32


def test_postings_slices_from_two_to_the_thirty_memberships(exe, monkeypatch):
    """Synthetic counts, no data.  4 keys of 5e8: n = 2e9, 2e9 // 9e8 + 1 = 3 slices, goals 666 666 666 and 1 333 333 332: the first
    key offsets at or above them are those of keys 2 and 3, so the slices hold 1e9, 5e8 and 5e8 memberships (all below 2^30).
    One key of 2^30 cannot be cut.  Two keys of 9e8: n // 9e8 + 1 = 3 slices for 2 keys; the cut for slice 1 (goal 6e8, key 1)
    is pulled back to 2 - 2 = 0 so that a key is left for each later slice: cuts 0, 0, 1, 2, an empty first slice, accepted.
    With two or more slices too many (KSP_SLICES=5) a range comes out negative and the job is refused as too large."""
    assert _postings(exe, monkeypatch, [500_000_000] * 4, [0]) == (0, {"devices": [0, 0, 0], "cuts": [0, 2, 3, 4], "sliced": True})
    assert _postings(exe, monkeypatch, [500_000_000] * 4, [0, 1]) == (0, {"devices": [0, 1, 0], "cuts": [0, 2, 3, 4], "sliced": True})
    assert _postings(exe, monkeypatch, [2**30], [0]) == (KSP_E_LIMIT, TOO_LARGE)
    assert _postings(exe, monkeypatch, [2**30 - 2, 2], [0]) == (0, {"devices": [0, 0], "cuts": [0, 1, 2], "sliced": True})
    assert _postings(exe, monkeypatch, [900_000_000] * 2, [0]) == (0, {"devices": [0, 0, 0], "cuts": [0, 0, 1, 2], "sliced": True})
    assert _postings(exe, monkeypatch, [900_000_000] * 2, [0], slices=5) == (KSP_E_LIMIT, TOO_LARGE)
    assert _postings(exe, monkeypatch, [900_000_000] * 72, [0]) == (KSP_E_LIMIT, "pairwise: more than 2^35 colour memberships")

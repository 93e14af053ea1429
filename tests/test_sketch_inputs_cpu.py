"""The generators of tests/sketch_inputs.py contain what they claim: a break straddling a tile edge, a reverse-palindromic k-mer,
a k-mer smaller and one larger than its reverse complement, duplicates within and across sources, a junction whose k-mers are
in neither source.  Plain Python over the restatement; no library call except the tile constant."""
import os

import pytest

import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine


def test_tile_constant_is_the_library_s():
    assert I.TILE == engine.SKETCH_TILE_BASES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kspider_amd.h")).read()
    assert f"#define KSP_SKETCH_TILE_BASES {I.TILE}u" in header


@pytest.mark.parametrize("k", [1, 21, 31, 33, 64])
def test_tile_edge_cases_have_their_lengths_and_breaks(k):
    cases = I.tile_edges(k)
    T = I.TILE
    assert sorted({c.offsets[1] for c in cases}) == sorted(set(I.tile_lengths(k)))
    seen = set()
    for c in cases:
        n = c.offsets[1]
        assert len(c.seq) == n and c.offsets == [0, n]
        breaks = [i for i, b in enumerate(c.seq) if chr(b) not in R.BASES]
        assert len(breaks) <= 1
        seen.add((n, breaks[0] if breaks else None))
        if breaks and k > 1 and n > T:
            # the windows the break kills straddle the edge between tile 0 and tile 1 (or lie against it)
            assert breaks[0] - (k - 1) < T <= breaks[0] + (k - 1) + 1
    for n in I.tile_lengths(k):
        for at in (None, T - 1, T, T + k - 2):
            assert ((n, at) in seen) == (at is None or at < n)
    # a break at tile - 1 and one at tile: the two sides of the edge; tile + k - 2: the last byte of the halo of tile 0's last window
    assert (2 * T + 1, T - 1) in seen and (2 * T + 1, T) in seen and (2 * T + 1, T + k - 2) in seen
    assert any(chr(b).islower() for b in cases[0].seq)


@pytest.mark.parametrize("k", [2, 31, 64])
def test_boundary_cases(k):
    T = I.TILE
    ends = []
    for c in I.boundaries(k):
        off = c.offsets
        assert off[0] == off[1] == 0 and off[-1] == off[-2] == len(c.seq)   # first and last sources are empty
        assert off[3] == off[4]                                             # and one in the middle
        assert 0 < off[3] - off[2] < k                                      # a source shorter than ksize
        assert all(chr(b) in R.BASES for b in c.seq)                        # no break byte marks a boundary
        ends.append(off[2])
    assert ends == [T - 1, T, T + 1]


@pytest.mark.parametrize("k", [21, 31])
def test_junction_spells_kmers_that_are_in_neither_source(k):
    c = I.junction(k)
    text = c.seq.decode()
    mid = c.offsets[1]
    inside = set()
    for s in range(2):
        inside |= {R.canonical(km) for _, km in R.source_kmers(c.seq[c.offsets[s]:c.offsets[s + 1]], k)}
    over = [R.canonical(text[p:p + k]) for p in range(mid - k + 1, mid)]
    assert len(over) == k - 1 and not (set(over) & inside)


@pytest.mark.parametrize("k", [2, 4, 32, 64])
def test_palindrome_is_its_own_reverse_complement(k):
    c, pal = I.palindrome(k)
    assert len(pal) == k and R.revcomp(pal) == pal and R.canonical(pal) == pal
    assert pal.encode() in c.seq


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 64])
def test_ordered_pair(k):
    c, small, large = I.ordered_pair(k)
    assert small < R.revcomp(small) == large and R.revcomp(large) == small
    assert c.seq == (small + large).encode() and c.offsets == [0, k, 2 * k]


@pytest.mark.parametrize("k", [1, 21, 64])
def test_duplicates(k):
    twice, shared, mirror = I.duplicates(k)
    kmers = [km for _, km in R.source_kmers(twice.seq, k)]
    assert len(kmers) == 2 * (400 - k + 1) and kmers[:len(kmers) // 2] == kmers[len(kmers) // 2:]
    a, b = (shared.seq[shared.offsets[s]:shared.offsets[s + 1]] for s in range(2))
    assert a == b and len(shared.offsets) == 3
    a, b = (mirror.seq[mirror.offsets[s]:mirror.offsets[s + 1]].decode() for s in range(2))
    assert R.revcomp(a) == b and a != b


def test_short_reads():
    one, many = I.short_reads()
    assert one.seq == many.seq and one.offsets == [0, len(one.seq)] and len(many.offsets) == 2001
    lengths = [many.offsets[i + 1] - many.offsets[i] - 1 for i in range(2000)]
    assert min(lengths) >= 40 and max(lengths) <= 150 and len(set(lengths)) > 50
    assert all(one.seq[o - 1:o] == b"\n" for o in many.offsets[1:])


def test_mixed_has_breaks_lower_case_and_uneven_sources():
    c = I.mixed()
    text = c.seq.decode("latin-1")
    assert any(ch.islower() and ch in R.BASES for ch in text)
    assert {"N", "\0", "\n"} <= set(text)
    assert len(c.offsets) == 4 and c.offsets[0] == 0 and c.offsets[-1] == len(c.seq) == 3000

"""dist.subtract_ranges: a range of the flat buffer minus the ranges other exchanges or updates cover, against the set
difference over the integers."""
import itertools

import pytest

from opensetgaitrecognition_pcaa_amd import dist as pdist


def _brute(lo, hi, covered):
    left = set(range(lo, hi))
    for a, b in covered:
        left -= set(range(a, b))
    return left


def _check(lo, hi, covered):
    got = pdist.subtract_ranges(lo, hi, covered)
    assert all(a < b for a, b in got), "non-empty ranges"
    assert all(p[1] < q[0] for p, q in zip(got, got[1:])), "sorted, disjoint, and merged where they touch"
    assert all(lo <= a and b <= hi for a, b in got)
    assert set(itertools.chain.from_iterable(range(a, b) for a, b in got)) == _brute(lo, hi, covered)
    return got


@pytest.mark.parametrize("covered,want", [
    ([], [(4, 20)]),                                            # empty cover
    ([(4, 6), (18, 20)], [(6, 18)]),                            # cover touching both ends
    ([(4, 20)], []),                                            # everything covered
    ([(12, 16), (5, 9), (8, 13)], [(4, 5), (16, 20)]),          # overlapping and unsorted
    ([(0, 3), (20, 25), (30, 31)], [(4, 20)]),                  # cover outside the range
    ([(0, 6), (18, 40)], [(6, 18)]),                            # cover reaching over the ends
    ([(6, 8), (8, 10), (10, 12)], [(4, 6), (12, 20)]),          # adjacent covers
    ([(7, 7), (9, 9)], [(4, 20)]),                              # empty covering ranges
])
def test_subtract_ranges_cases(covered, want):
    assert _check(4, 20, covered) == want


def test_subtract_ranges_vs_brute_force_over_small_integers():
    spans = [(a, b) for a in range(0, 9) for b in range(a, 9)]
    for covered in itertools.chain(itertools.combinations(spans, 1), itertools.combinations(spans[::3], 2),
                                   itertools.combinations(spans[::7], 3)):
        for lo, hi in ((2, 7), (0, 8), (3, 3)):
            _check(lo, hi, list(covered))
            _check(lo, hi, list(reversed(covered)))


def test_subtract_ranges_of_the_trainer_s_two_uses():
    """the residual all-reduces (region minus fused and bucketed ranges) and the side-stream Adam (a pending chunk minus the
    fused ranges), at offsets shaped like the flat buffer's: 64-float aligned, the wide weights at the end"""
    dec_start, total = 1024, 8192
    fused = [(4096, 6144), (2048, 4096)]
    assert _check(dec_start, total, fused + [(6144, 8192)]) == [(1024, 2048)]
    assert _check(dec_start, total, fused) == [(1024, 2048), (6144, 8192)]
    assert _check(max(0, dec_start), 2048, fused) == [(1024, 2048)]
    assert _check(6144, 8192, []) == [(6144, 8192)]

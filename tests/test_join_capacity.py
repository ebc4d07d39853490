"""The capacity the pile-up join's hit buffer starts with (dh_join_hit_capacity, host arithmetic -- no GPU needed).

Hits per base grow with pile-up depth (about n p^2 / 2 for n reads whose k-mers survive with probability p), so the
buffer is sized by sum(bases x reads) x rate x 1.5, never below the earlier max(2^20, 1.25 x bases), never above a quarter
of the free device memory (that floor apart)."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import join_hit_capacity

RATE0, MARGIN, MEM_FRACTION = 0.0128, 1.5, 0.25


def old_capacity(total):
    return max(1 << 20, int(1.25 * total))


def test_headline_part_fits_without_a_rerun():
    """A part of the headline process stage: 333 pile-ups of 166 reads cropped to 2 512 bases produce 1.94 hits per base."""
    bases, reads = [166 * 2512] * 333, [166] * 333
    total = sum(bases)
    cap = join_hit_capacity(bases, reads, skip_self=2)
    assert 1.94 * total <= cap <= 4 * total
    assert abs(cap - RATE0 * MARGIN * 166 * total) <= 1


CASES = [
    ([], []),                                  # no group at all
    ([0], [0]),                                # one empty group
    ([0, 0, 5000, 0], [0, 0, 3, 0]),           # empty group ids around a small pile-up
    ([1000], [1]),                             # a single group of one read
    ([60 * 6000], [60]),                       # a single group
    ([2_000_000], [2]),                        # shallow and long: the depth term is far below 1.25 x bases
    ([400 * 10_000] * 50, [400] * 50),         # deep
    ([30 * 900, 166 * 2512, 1, 512 * 20000], [30, 166, 1, 512]),
]


@pytest.mark.parametrize("bases,reads", CASES)
def test_never_below_the_earlier_constant(bases, reads):
    for skip_self in (0, 1, 2):
        for rate in (0.0, 1e-6, RATE0, 0.4):
            for free_bytes in (-1, 0, 1 << 20, 1 << 34):
                assert join_hit_capacity(bases, reads, skip_self, rate, free_bytes) >= old_capacity(sum(bases))


def test_monotone_in_the_learned_rate():
    bases, reads = [166 * 2512] * 20, [166] * 20
    rates = [1e-5, 1e-3, RATE0, 0.02, 0.1, 0.375, 1.0, 5.0]
    caps = [join_hit_capacity(bases, reads, 2, r) for r in rates]
    assert all(a <= b for a, b in zip(caps, caps[1:]))
    assert caps[0] == old_capacity(sum(bases)) and caps[-1] > caps[2] > caps[0]
    # a rate of zero or below means "not learned yet": the initial figure
    assert join_hit_capacity(bases, reads, 2, 0.0) == join_hit_capacity(bases, reads, 2, -1.0) == caps[2]


@pytest.mark.parametrize("skip_self", [0, 1])
def test_both_directions_of_a_pair_double_the_expectation(skip_self):
    bases, reads = [166 * 2512] * 20 + [60 * 6000], [166] * 20 + [60]
    one = join_hit_capacity(bases, reads, 2)
    assert one > old_capacity(sum(bases))  # the depth term decides, not the floor
    assert abs(join_hit_capacity(bases, reads, skip_self) - 2 * one) <= 1


def test_memory_clamp():
    bases, reads = [166 * 2512] * 333, [166] * 333
    total, free = sum(bases), 8 << 30
    want = join_hit_capacity(bases, reads, 2)
    limit = int(MEM_FRACTION * free) // 8
    assert old_capacity(total) < limit < want
    assert join_hit_capacity(bases, reads, 2, free_bytes=free) == limit
    # learning does not lift it
    assert join_hit_capacity(bases, reads, 2, rate=1.0, free_bytes=free) == limit
    # enough memory: no effect; next to none: the earlier constant, which the rerun then corrects
    assert join_hit_capacity(bases, reads, 2, free_bytes=1 << 40) == want
    assert join_hit_capacity(bases, reads, 2, free_bytes=1 << 20) == old_capacity(total)


def test_binding_checks_its_arguments_and_the_library_exports_the_counters():
    with pytest.raises(ValueError):
        join_hit_capacity([1, 2], [1])
    assert hasattr(dentist_amd.lib(), "dh_get_join_counts") and hasattr(dentist_amd.Context, "join_counts")
    assert join_hit_capacity(np.asarray([5000], dtype=np.int32), np.asarray([3], dtype=np.int64)) == 1 << 20

"""The placement rule of the pair ensemble kernel on its NumPy model alone (tests/place_numpy.py): every half step's assignment
is a permutation of the pairs with at most n0 / 8 items per XCD class, and at least 90 % of the items that prefer a class
get it (a floor against a broken rule: capacity n0 / 8 per class against a binomial demand leaves about 6 % over)."""
import numpy as np
import pytest

from place_numpy import SEG, eligible, place_chunk, stretch_draws


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_headline_width(seed):
    W, K = 256, 600
    n0 = W // 2
    order, cw = stretch_draws(np.random.RandomState(seed), W, K)
    place, n_pref, n_hit = place_chunk(order, cw)
    for t in range(K):
        for lo in (0, n0):
            p = place[t, lo:lo + n0]
            assert sorted(p.tolist()) == list(range(n0))
            assert np.bincount(p % 8, minlength=8).max() <= n0 // 8
    # every item prefers a class but those of a segment's first half step and the first-half items with no fresh row (a quarter)
    assert n_pref > 0.95 * (0.5 + 0.5 * 0.75 * (1 - 1 / SEG)) * K * W
    print("preferred", n_pref, "placed on it", n_hit, n_hit / n_pref)
    assert n_hit >= 0.90 * n_pref


def test_capacity_one_and_segment_heads():
    """W = 16: one pair per class, every conflict goes to the leftovers; the first half step of a segment is the identity."""
    W, K = 16, 3 * SEG + 5
    order, cw = stretch_draws(np.random.RandomState(7), W, K)
    place, n_pref, n_hit = place_chunk(order, cw)
    for t in range(K):
        for lo in (0, 8):
            assert sorted(place[t, lo:lo + 8].tolist()) == list(range(8))
        if t % SEG == 0:
            assert place[t, :8].tolist() == list(range(8))
    assert 0 < n_hit < n_pref


def test_eligible_widths():
    assert eligible(16) and eligible(64) and eligible(256)
    assert not eligible(20) and not eligible(15) and not eligible(17) and not eligible(512)

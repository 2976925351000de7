"""NumPy statement of the placement rule of the pair ensemble kernel (alabi_amd/csrc/ens_place.hip).

A chunk of K steps is cut into segments of SEG steps that are placed independently.  Within a segment, for the items of a half
step in list order: an item prefers the XCD class (pair % 8) that made its fresh input row -- one fresh row: that row's class;
both fresh: the partner's; none: no preference.  A row is fresh iff its walker was updated in the half step just before: the
partner's always in a second half step; in a first half step the rows of the walkers of the previous step's second list
(none in the first step of a segment).  An item gets its preferred class while that class has fewer than n0 / 8 items (and
there the lowest free pair); the items left over take the free pairs in ascending order."""
import numpy as np

SEG = 4


def eligible(W):
    n0 = (W + 1) // 2
    return W == 2 * n0 and n0 % 8 == 0 and n0 <= 128


def place_half(own, partner, fresh, cls_of, n0):
    """Pairs of one half step's items.  own, partner: walker ids by list position; fresh: set of walkers whose row is fresh;
    cls_of: walker -> class that made its newest row.  Returns (pair by list position, items with a preference, items on it)."""
    cap = n0 // 8
    count = [0] * 8
    pair = [-1] * n0
    n_pref = n_hit = 0
    for i in range(n0):
        w, c = int(own[i]), int(partner[i])
        pref = cls_of[c] if c in fresh else cls_of[w] if w in fresh else None
        if pref is None:
            continue
        n_pref += 1
        if count[pref] < cap:
            pair[i] = pref + 8 * count[pref]
            count[pref] += 1
            n_hit += 1
    free = [p for p in range(n0) if p // 8 >= count[p % 8]]
    left = [i for i in range(n0) if pair[i] < 0]
    assert len(free) == len(left)
    for i, p in zip(left, free):
        pair[i] = p
    return pair, n_pref, n_hit


def place_chunk(order, cw, seg=SEG):
    """order, cw: [K, W] walker and partner (ids within the ensemble) by list position, first list then second.
    Returns (place [K, W]: the pair of every item, items with a preference, items placed on it)."""
    order, cw = np.asarray(order), np.asarray(cw)
    K, W = order.shape
    n0 = W // 2
    assert eligible(W)
    place = np.zeros((K, W), dtype=np.int32)
    n_pref = n_hit = 0
    cls_of = {}
    for t in range(K):
        for half in (0, 1):
            lo = half * n0
            if half == 1:
                fresh = set(int(x) for x in order[t, :n0])
            elif t % seg == 0:
                fresh = set()
            else:
                fresh = set(int(x) for x in order[t - 1, n0:])
            pair, a, b = place_half(order[t, lo:lo + n0], cw[t, lo:lo + n0], fresh, cls_of, n0)
            for i in range(n0):
                cls_of[int(order[t, lo + i])] = pair[i] % 8
            place[t, lo:lo + n0] = pair
            n_pref += a
            n_hit += b
    return place, n_pref, n_hit


def stretch_draws(rng, W, K):
    """Lists and partners as the stretch move draws them: a random split into two lists of W / 2, every item's partner uniform
    in the other list."""
    n0 = W // 2
    order = np.stack([rng.permutation(W) for _ in range(K)])
    cw = np.empty_like(order)
    for t in range(K):
        cw[t, :n0] = order[t, n0 + rng.randint(0, W - n0, n0)]
        cw[t, n0:] = order[t, rng.randint(0, n0, W - n0)]
    return order, cw

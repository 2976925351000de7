#!/usr/bin/env python3
"""Generate tests/golden/ndtri_truth.npz: the inverse normal CDF at the grid of the device accuracy test, to 40 digits.

    python tests/golden/make_golden_ndtri.py        (needs mpmath)

For every grid value u (a double, taken exactly) the root z of ncdf(z) = u is found with mpmath.findroot at 40 digits, started
from scipy.special.ndtri(u); below u = 1/2 the equation is solved as ncdf(z) = u, above it as ncdf(-z) = 1 - u (1 - u formed in
mpmath, exactly), so that neither tail loses digits.  Stored: u [n] and truth [n], the root rounded to the nearest double.

Grid (about 100 values): 2^-54, 1e-300, 1e-100, 1e-20; logspace(-16, -1, 46); the branch points of AS 241 / Cephes 0.02425
(+- 1e-12), 0.075, 0.425, 0.5 (+- 1e-9), 0.575, 0.925, 0.97575; 1 - logspace(-1, -15.9, 40); 1 - 2^-53.
"""
import os

import mpmath as mp
import numpy as np
from scipy.special import ndtri

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ndtri_truth.npz")


def grid():
    u = [2.0 ** -54, 1e-300, 1e-100, 1e-20]
    u += list(np.logspace(-16, -1, 46))
    u += [0.02425 - 1e-12, 0.02425, 0.02425 + 1e-12, 0.075, 0.425, 0.5 - 1e-9, 0.5, 0.5 + 1e-9, 0.575, 0.925, 0.97575]
    u += list(1.0 - np.logspace(-1, -15.9, 40))
    u += [1.0 - 2.0 ** -53]
    return np.array(u, dtype=np.float64)


def truth(u):
    mp.mp.dps = 40
    um = mp.mpf(float(u))
    z0 = mp.mpf(float(ndtri(u)))
    if u == 0.5:
        return 0.0
    tail = um if u < 0.5 else 1 - um                       # the probability of the nearer tail, exact
    w = mp.findroot(lambda w: mp.log(mp.ncdf(w)) - mp.log(tail), z0 if u < 0.5 else -z0)     # w <= 0: ncdf(w) = tail
    assert abs(mp.ncdf(w) / tail - 1) <= mp.mpf(10) ** -35, (u, w)
    return float(w if u < 0.5 else -w)


def main():
    u = grid()
    t = np.array([truth(x) for x in u])
    np.savez_compressed(OUT, u=u, truth=t)
    err = np.abs(ndtri(u) - t) / np.maximum(1.0, np.abs(t))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(u), "values; scipy's error", err.max())


if __name__ == "__main__":
    main()

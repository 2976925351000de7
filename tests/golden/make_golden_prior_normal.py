#!/usr/bin/env python3
"""Generate tests/golden/reference_prior_normal_vectors.npz by EXECUTING the reference's alabi/utility.py.

    python tests/golden/make_golden_prior_normal.py <path to the reference's alabi directory>

utility.py is loaded by file path, as make_golden_metrics.py loads metrics.py; where scikit-optimize is not installed its
imports (used by prior_sampler only, which is not called here) are satisfied by inert placeholder modules.  Nothing from the
reference is copied: this script stores INPUTS and the OUTPUTS the reference's prior_transform_normal returned.

Vectors written (float64):
  bounds [4,2], data [4,2] (NaN = (None, None))   the mixed prior: coordinates 1 and 3 normal
  x1 [4], out1 [4]                                one 1-D call
  x2 [33,4], out2 [33,4]                          one 2-D call (cube points strictly inside (0, 1), a few near the ends)
"""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_prior_normal_vectors.npz")


def _placeholder_skopt():
    try:
        import skopt  # noqa: F401
        return
    except ImportError:
        pass
    for name, attrs in (("skopt", ()), ("skopt.space", ("Space",)), ("skopt.space.space", ("Real",)),
                        ("skopt.sampler", ("Sobol", "Lhs", "Halton", "Hammersly", "Grid"))):
        mod = types.ModuleType(name)
        mod.__path__ = []
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod


def main(ref):
    _placeholder_skopt()
    spec = importlib.util.spec_from_file_location("alabi_ref_utility", os.path.join(ref, "utility.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.RandomState(20261017)
    bounds = np.array([[-2.0, 2.0], [0.0, 10.0], [3.0, -1.0], [-50.0, 50.0]])
    data = [(None, None), (5.0, 1.0), (None, None), (-0.25, 12.5)]
    x1 = rng.rand(4)
    x2 = rng.rand(33, 4)
    x2[0], x2[1], x2[2] = 1e-12, 1.0 - 1e-12, 0.5
    out = dict(bounds=bounds, data=np.array([[np.nan if v is None else v for v in dd] for dd in data]), x1=x1, x2=x2,
               out1=mod.prior_transform_normal(x1, bounds, data), out2=mod.prior_transform_normal(x2, bounds, data))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

"""Proposal moves of the ensemble sampler: emcee's ``EnsembleSampler(moves=...)``.

The reference documents ``sampler_kwargs['moves']`` ("Custom proposal moves", alabi/core.py:2144) and hands it to
``emcee.EnsembleSampler`` (alabi/core.py:2319).  Three moves run on the GPU here, alone or as a weighted mixture from which
ONE move is chosen per step, as emcee does:

* ``StretchMove(a=2.0)``        -- emcee 3 ``moves/stretch.py`` (the default);
* ``DEMove(sigma, gamma0)``     -- emcee 3 ``moves/de.py``: q = s + gamma (C[j2] - C[j1]) with two distinct walkers of the
  complementary set and gamma = gamma0 (1 + sigma n), n standard normal; gamma0 defaults to 2.38 / sqrt(2 ndim);
* ``SnookerMove(gammas=1.7)``   -- the snooker update of ter Braak & Vrugt (2008, eq. 4) on the sampler's two-way split: three
  distinct walkers z, z1, z2 of the complementary set, e the unit vector from z to s, q = s + gammas (e.z1 - e.z2) e, log
  factor (ndim - 1) (ln|q - z| - ln|s - z|).  Typically mixed with DE: ``[(DEMove(), 0.8), (SnookerMove(), 0.2)]``.

``parse_moves`` is pure host code (no GPU, no library): it accepts what emcee accepts -- None, one move, a list of moves, a
list of (move, weight) pairs -- and recognises this module's classes as well as foreign ``StretchMove`` / ``DEMove`` objects by
class name and attributes, so real ``emcee.moves`` objects of these two classes work where emcee is installed.  Every other
move raises ``NotImplementedError``; that includes emcee's ``DESnookerMove``, which stands for different arithmetic (half the
published log factor, a four-way split): ask for ``SnookerMove`` instead.
"""
from __future__ import annotations

import numpy as np

__all__ = ["StretchMove", "DEMove", "SnookerMove", "MoveSet", "parse_moves", "MAX_MOVES", "KIND_STRETCH", "KIND_DE",
           "KIND_SNOOKER"]

MAX_MOVES = 8                    # ALABI_MAX_MOVES of the library: the table travels in the draw kernel's arguments
KIND_STRETCH, KIND_DE, KIND_SNOOKER = 0, 1, 2


class StretchMove:
    """Goodman & Weare stretch move with scale ``a`` (emcee.moves.StretchMove)."""

    def __init__(self, a=2.0):
        self.a = float(a)
        if not (self.a > 1.0 and np.isfinite(self.a)):
            raise ValueError("StretchMove needs a > 1")

    def __repr__(self):
        return f"StretchMove(a={self.a})"


class DEMove:
    """Differential-evolution move (emcee.moves.DEMove; Nelson et al. 2013, ter Braak 2006).  ``gamma0=None`` means
    2.38 / sqrt(2 ndim); mix in a ``DEMove(gamma0=1.0)`` at a small weight to let walkers jump between modes."""

    def __init__(self, sigma=1.0e-5, gamma0=None):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        if not np.isfinite(self.sigma) or (self.gamma0 is not None and not np.isfinite(self.gamma0)):
            raise ValueError("DEMove needs finite sigma and gamma0")

    def __repr__(self):
        return f"DEMove(sigma={self.sigma}, gamma0={self.gamma0})"


class SnookerMove:
    """Snooker update (ter Braak & Vrugt 2008, eq. 4) with the fixed step ``gammas`` along the line through the walker and a
    walker of the complementary set.  Not emcee's ``DESnookerMove``: the log factor is the published one."""

    def __init__(self, gammas=1.7):
        self.gammas = float(gammas)
        if not np.isfinite(self.gammas):
            raise ValueError("SnookerMove needs a finite gammas")

    def __repr__(self):
        return f"SnookerMove(gammas={self.gammas})"


def _table_row(m, ndim):
    """(kind, p0, p1) of a move in the library's table."""
    if isinstance(m, DEMove):
        return KIND_DE, 2.38 / np.sqrt(2 * ndim) if m.gamma0 is None else m.gamma0, m.sigma
    if isinstance(m, SnookerMove):
        return KIND_SNOOKER, m.gammas, 0.0
    return KIND_STRETCH, m.a, 0.0


class MoveSet:
    """A parsed move set: ``moves`` (this module's objects), normalised ``weights`` and the table the library takes --
    ``kind``, ``cum`` = np.cumsum(w / w.sum()), ``p0`` (a | gamma0 with its default resolved | gammas), ``p1`` (0 | sigma | 0)."""

    def __init__(self, moves, weights, ndim):
        self.moves = list(moves)
        w = np.asarray(weights, dtype=np.float64)
        self.weights = w / w.sum()
        self.cum = np.cumsum(w / w.sum())
        rows = [_table_row(m, ndim) for m in self.moves]
        self.kind = np.array([r[0] for r in rows], dtype=np.int32)
        self.p0 = np.array([r[1] for r in rows], dtype=np.float64)
        self.p1 = np.array([r[2] for r in rows], dtype=np.float64)

    @property
    def has_de(self):
        return bool(np.any(self.kind == KIND_DE))

    @property
    def has_snooker(self):
        return bool(np.any(self.kind == KIND_SNOOKER))

    @property
    def multi_partner(self):
        """Some move reads more than one partner row (DE, snooker): one launch per half step, no sharding."""
        return self.has_de or self.has_snooker

    def __len__(self):
        return len(self.moves)


def _as_move(obj):
    """This module's move for ``obj``: one of its own, or a foreign object recognised by class name and attributes."""
    if isinstance(obj, (StretchMove, DEMove, SnookerMove)):
        return obj
    name = type(obj).__name__
    if name == "StretchMove" and hasattr(obj, "a"):
        return StretchMove(a=obj.a)
    if name == "DEMove" and hasattr(obj, "sigma") and hasattr(obj, "gamma0"):
        return DEMove(sigma=obj.sigma, gamma0=obj.gamma0)
    hint = ""
    if name == "DESnookerMove":
        hint = ("; emcee's DESnookerMove stands for different arithmetic (half the published log factor, a four-way split) -- "
                "use alabi_amd.moves.SnookerMove, the published snooker update")
    raise NotImplementedError(f"move {name} is not available on the GPU: the ensemble sampler runs StretchMove, DEMove, "
                              f"alabi_amd.moves.SnookerMove and weighted mixtures of them{hint}")


def parse_moves(moves, ndim):
    """``moves`` as emcee's EnsembleSampler takes it -> ``MoveSet``, or None for None (the default stretch move)."""
    if moves is None:
        return None
    if isinstance(moves, (list, tuple)):
        items = list(moves)
        if not items:
            raise ValueError("moves must not be empty")
        if all(isinstance(it, (list, tuple)) and len(it) == 2 for it in items):
            objs, weights = [it[0] for it in items], [float(it[1]) for it in items]
        else:
            objs, weights = items, [1.0] * len(items)
    else:
        objs, weights = [moves], [1.0]
    parsed = [_as_move(o) for o in objs]
    w = np.asarray(weights, dtype=np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not (w.sum() > 0.0):
        raise ValueError("move weights must be non-negative, finite and not all zero")
    if len(parsed) > MAX_MOVES:
        raise ValueError(f"at most {MAX_MOVES} moves in a mixture")
    return MoveSet(parsed, w, int(ndim))

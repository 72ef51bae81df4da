"""Tabulated pair potentials, host side of nl_set_pair_table (include/nl_hip.h).

numpy only: importable without the HIP library.  A table samples F(r) = -U'(r) / r (the force over r) and U(r) at knots
uniform in r^2, ``x_k = r_min^2 + k D`` with ``D = (r_max^2 - r_min^2) / (nknots - 1)``; a pair at r^2 reads the segment it
falls into and interpolates linearly in r^2.  ``F`` and ``U`` are ``(nknots,)`` for one table or ``(nslots, nknots)`` with
the row ``rdf.slot(a, b, ntypes)`` per unordered pair of types.
"""
from __future__ import annotations

import numpy as np


def spacing(r_min, r_max, nknots):
    """D, the distance of two knots in r^2."""
    return (float(r_max) ** 2 - float(r_min) ** 2) / (int(nknots) - 1)


def knots(r_min, r_max, nknots):
    """r at the knots: sqrt(r_min^2 + k D), k = 0 .. nknots - 1 (float64)."""
    if not (0 < r_min < r_max) or nknots < 2:
        raise ValueError("a table needs 0 < r_min < r_max and nknots >= 2")
    return np.sqrt(float(r_min) ** 2 + np.arange(int(nknots), dtype=np.float64) * spacing(r_min, r_max, nknots))


def sample(u, du_dr, r_min, r_max, nknots):
    """``(F, U)`` of a potential given by float64 callables u(r) and du_dr(r) = U'(r): F = -U'(r) / r and U at the knots."""
    r = knots(r_min, r_max, nknots)
    F = -np.asarray(du_dr(r), dtype=np.float64) / r
    U = np.asarray(u(r), dtype=np.float64) + 0.0 * r
    return F, U


def interpolate(F, U, r_min, r_max, r2):
    """``(fr, pe, in)`` of the rule of nl_set_pair_table in float64 for an array of r^2 (one row of a table: F, U of
    ``(nknots,)``).  in = 0 < r2 < r_max^2; outside it fr = pe = 0; inside it, with s = (r2 - r_min^2) / D,
    k = min(int(s), nknots - 2) and t = s - k: fr = F_k + t (F_{k+1} - F_k), pe likewise; NaN below r_min^2.  The force on i
    is fr (r_i - r_j)."""
    F, U = np.asarray(F, dtype=np.float64), np.asarray(U, dtype=np.float64)
    if F.ndim != 1 or F.shape != U.shape or len(F) < 2:
        raise ValueError("interpolate takes one row of a table: F and U of (nknots,)")
    r2 = np.asarray(r2, dtype=np.float64)
    nk = len(F)
    x0, xc = float(r_min) ** 2, float(r_max) ** 2
    inn = (r2 < xc) & (r2 > 0)
    below = inn & (r2 < x0)
    s = (r2 - x0) * (1.0 / spacing(r_min, r_max, nk))
    k = np.where(inn & ~below, np.minimum(np.where(inn & ~below, s, 0.0).astype(np.int64), nk - 2), 0)
    t = s - k
    dF, dU = np.append(np.diff(F), 0.0), np.append(np.diff(U), 0.0)
    fr = np.where(inn, np.where(below, np.nan, F[k] + t * dF[k]), 0.0)
    pe = np.where(inn, np.where(below, np.nan, U[k] + t * dU[k]), 0.0)
    return fr, pe, inn

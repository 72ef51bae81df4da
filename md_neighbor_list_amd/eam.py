"""Embedded-atom potentials, host side of nl_set_eam (include/nl_hip.h).

numpy only: importable without the HIP library.  E = sum_i F_{t_i}(rho_i) + sum_pairs phi(r), rho_i = sum_j f_{t_j}(r_ij).
The pair part phi is a table of ``pair_table``.  A density table samples ``f_b(r)`` and ``G_b = -f_b'(r) / r`` at the knots of
``pair_table.knots(r_min, r_max, nknots_d)``, uniform in r^2, one row per type b of the source particle; an embedding table
samples ``F_a(rho)`` and ``F_a'(rho)`` at ``rho_k = k rho_max / (nknots_e - 1)``, one row per type a.  ``density`` and
``embed`` are the interpolation rule in float64: the tests' reference and a user's inspection tool, as
``pair_table.interpolate`` is.
"""
from __future__ import annotations

import numpy as np

from . import pair_table


def rho_knots(rho_max, nknots):
    """rho at the knots of an embedding table: k Drho, k = 0 .. nknots - 1 (float64)."""
    if not rho_max > 0 or nknots < 2:
        raise ValueError("an embedding table needs rho_max > 0 and nknots >= 2")
    return np.arange(int(nknots), dtype=np.float64) * (float(rho_max) / (int(nknots) - 1))


def _each(fn):
    return list(fn) if isinstance(fn, (list, tuple)) else [fn]


def sample(f, df_dr, F, dF_drho, r_min, r_max, nknots_d, rho_max, nknots_e):
    """``(f, G, E, P)`` for nl_set_eam from float64 callables: f(r) and df_dr(r) = f'(r) give ``f`` and ``G = -f'(r) / r`` at the
    density knots, F(rho) and dF_drho(rho) give ``E`` and ``P`` at the embedding knots, rho = 0 included (a callable that is
    singular there, as sqrt(rho) is, must be regularised by the caller).  Each argument is one callable (one type: arrays of
    ``(nknots,)``) or a sequence of ntypes callables (``(ntypes, nknots)``)."""
    r, rho = pair_table.knots(r_min, r_max, nknots_d), rho_knots(rho_max, nknots_e)
    fs, dfs, Fs, dFs = _each(f), _each(df_dr), _each(F), _each(dF_drho)
    if not len(fs) == len(dfs) == len(Fs) == len(dFs):
        raise ValueError("f, df_dr, F and dF_drho need one callable per type each")
    fv = np.stack([np.asarray(c(r), dtype=np.float64) + 0.0 * r for c in fs])
    G = np.stack([-np.asarray(c(r), dtype=np.float64) / r for c in dfs])
    E = np.stack([np.asarray(c(rho), dtype=np.float64) + 0.0 * rho for c in Fs])
    P = np.stack([np.asarray(c(rho), dtype=np.float64) + 0.0 * rho for c in dFs])
    if not isinstance(f, (list, tuple)):
        return fv[0], G[0], E[0], P[0]
    return fv, G, E, P


def density(f, G, r_min, r_max, r2):
    """``(f, G, in)`` of one density slot (f, G of ``(nknots,)``) at an array of r^2, the rule of nl_set_eam in float64: the grid
    rule of ``pair_table.interpolate`` with in = 0 < r2 < r_max^2, 0 outside it and NaN below r_min^2."""
    Gv, fv, inn = pair_table.interpolate(G, f, r_min, r_max, r2)
    return fv, Gv, inn


def embed(E, P, rho_max, rho):
    """``(Fe, fp)`` of one embedding slot (E, P of ``(nknots,)``) at an array of rho, the rule of nl_set_eam in float64:
    s = rho / Drho, k = min(int(s), nknots - 2), t = s - k, Fe = E_k + t (E_{k+1} - E_k), fp likewise; NaN for rho outside
    [0, rho_max] or NaN."""
    E, P = np.asarray(E, dtype=np.float64), np.asarray(P, dtype=np.float64)
    if E.ndim != 1 or E.shape != P.shape or len(E) < 2:
        raise ValueError("embed takes one row of a table: E and P of (nknots,)")
    rho = np.asarray(rho, dtype=np.float64)
    nk = len(E)
    ok = (rho >= 0) & (rho <= float(rho_max))
    s = np.where(ok, rho, 0.0) * (1.0 / (float(rho_max) / (nk - 1)))
    k = np.minimum(s.astype(np.int64), nk - 2)
    t = s - k
    dE, dP = np.append(np.diff(E), 0.0), np.append(np.diff(P), 0.0)
    return np.where(ok, E[k] + t * dE[k], np.nan), np.where(ok, P[k] + t * dP[k], np.nan)

"""Dissipative particle dynamics, host side of nl_set_dpd (include/nl_hip.h).

numpy and the standard library only: importable without the HIP library.  The DPD pair term is
``F_ij = [-gamma w(r)^2 (e_ij . v_ij) + sigma w(r) xi_ij / sqrt(dt)] e_ij``; the library takes the weight as one table
``A = w(r) / r`` at the knots ``pair_table.knots(r_min, r_max, nknots)``, uniform in r^2 (``weight``), squares the interpolated
A for the friction, and draws ``xi_ij`` from a hash of (seed, step, min(i, j), max(i, j)) in 64-bit integers, which
``pair_noise_int`` and ``pair_noise`` restate here in numpy.  ``conservative`` samples the soft repulsion of DPD proper for
``NeighListGPU.set_pair_table``; ``sigma_for`` is the fluctuation-dissipation relation.
"""
from __future__ import annotations

import math

import numpy as np

from . import pair_table

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
XI_SCALE = math.sqrt(3.0) / 2.0 ** 24


def weight(r_min, r_max, nknots, s=1.0):
    """``A = w(r) / r`` at the knots, ``w = (1 - r / r_max)^s``: s = 1 is Groot and Warren's weight (the friction's is its
    square), other s the generalised weights that tune the Schmidt number.  The last knot (r = r_max) is exactly 0."""
    r = pair_table.knots(r_min, r_max, nknots)
    w = np.maximum(1.0 - r / float(r_max), 0.0) ** float(s)
    w[-1] = 0.0
    return w / r


def conservative(a, r_c, r_min, r_max, nknots):
    """``(F, U)`` of the soft repulsion ``U = a r_c (1 - r / r_c)^2 / 2`` inside r_c, 0 beyond: ``F = -U'(r) / r =
    a (1 - r / r_c) / r``, at the knots, for ``set_pair_table``."""
    r = pair_table.knots(r_min, r_max, nknots)
    x = np.maximum(1.0 - r / float(r_c), 0.0)
    return float(a) * x / r, 0.5 * float(a) * float(r_c) * x * x


def sigma_for(gamma, kT):
    """The noise amplitude of the fluctuation-dissipation relation: ``sigma = sqrt(2 gamma kT)`` (arrays: per slot)."""
    return np.sqrt(2.0 * np.asarray(gamma, dtype=np.float64) * float(kT))


def fin(z):
    """The finaliser of the pair noise on uint64 arrays, modulo 2^64."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= _M1
        z ^= z >> np.uint64(27)
        z *= _M2
        z ^= z >> np.uint64(31)
    return z


def pair_key(seed, step):
    """``fin(fin(seed) + step)`` of a call, a uint64 scalar."""
    with np.errstate(over="ignore"):
        s = fin(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)) + np.uint64(int(step) & 0xFFFFFFFFFFFFFFFF)
    return fin(s)[0]


def pair_noise_int(i, j, seed, step):
    """The integer of the pair noise, ``2 m + 1 - 2^24`` with m the top 24 bits of ``fin(key + (lo << 32 | hi))``, lo and hi
    the smaller and the larger of the rows i and j (arrays broadcast): int64, odd, below 2^24 in magnitude, symmetric in
    (i, j)."""
    i, j = np.broadcast_arrays(np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64))
    lo, hi = np.minimum(i, j) & np.uint64(0xFFFFFFFF), np.maximum(i, j) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        z = fin(pair_key(seed, step) + ((lo << np.uint64(32)) | hi))
    m = (z >> np.uint64(40)).astype(np.int64)
    return 2 * m + 1 - (1 << 24)


def pair_noise(i, j, seed, step, dtype=np.float64):
    """``xi_ij``: the integer in ``dtype`` (exact) times ``sqrt(3) / 2^24`` rounded to ``dtype``; uniform, zero mean, unit
    variance."""
    dt = np.dtype(dtype).type
    return pair_noise_int(i, j, seed, step).astype(dt) * dt(XI_SCALE)


def interpolate(A, r_min, r_max, r2):
    """``(a, in)`` of the rule of nl_set_dpd in float64 for an array of r^2: pair_table.interpolate on the weight table.  The
    friction of a pair is ``-gamma a^2 (d . dv) d``, its noise ``sigma / sqrt(dt) a xi d``; NaN below r_min^2, 0 outside
    ``in``."""
    A = np.asarray(A, dtype=np.float64)
    a, _, inn = pair_table.interpolate(A, np.zeros_like(A), r_min, r_max, r2)
    return a, inn

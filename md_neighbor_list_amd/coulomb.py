"""Short-range electrostatics, host side of nl_set_coulomb_table (include/nl_hip.h).

numpy and the standard library only: importable without the HIP library.  The charge term of a pair is ``q_i q_j C(r)``; a
sampler returns ``(K, C)`` with ``C = C(r)`` and ``K = -C'(r) / r`` at the knots ``pair_table.knots(r_min, r_max, nknots)``,
uniform in r^2, ready for ``NeighListGPU.set_coulomb_table``.  ``prefactor`` multiplies both: the Coulomb constant over the
dielectric in the caller's units (1 in Gaussian / reduced units, 332.06371 kcal A / (mol e^2), 138.935458 kJ nm / (mol e^2)).

The correction an Ewald / PME sum owes for the bonded pairs that nl_set_exclusions removed is a sum over the exclusion table
with a table of its own (nl_set_coul_excl_table, ``NeighListGPU.set_excluded_coulomb_table``): ``ewald_excluded`` samples it, and
``ewald_self`` is the self-energy ``-alpha / sqrt(pi) sum q_i^2``, a host scalar.  What is not here is no pair sum at all: the
reciprocal-space sum of Ewald / PME and the net-charge term.
"""
from __future__ import annotations

import math

import numpy as np

from . import pair_table

_TWO_OVER_SQRT_PI = 2.0 / math.sqrt(math.pi)


def _erfc(x):
    return np.array([math.erfc(v) for v in np.asarray(x, dtype=np.float64).ravel()]).reshape(np.shape(x))


def _damped(alpha, r):
    """(erfc(alpha r) / r, its force erfc(alpha r) / r^2 + 2 alpha / sqrt(pi) exp(-alpha^2 r^2) / r)."""
    e = _erfc(alpha * r)
    return e / r, e / (r * r) + _TWO_OVER_SQRT_PI * alpha * np.exp(-(alpha * r) ** 2) / r


def _out(prefactor, force, c):
    return float(prefactor) * force, float(prefactor) * c


def ewald_real(alpha, r_min, r_max, nknots, prefactor=1.0):
    """The real-space part of Ewald / PME: C = erfc(alpha r) / r, neither shifted nor switched at r_max."""
    r = pair_table.knots(r_min, r_max, nknots)
    c, f = _damped(float(alpha), r)
    return _out(prefactor, f / r, c)


def ewald_excluded(alpha, r_min, r_max, nknots, prefactor=1.0):
    """The term of an excluded pair under Ewald / PME, whose reciprocal sum still contains it: C = -erf(alpha r) / r (the sign
    belongs to the table), K = -C'(r) / r = 2 alpha / sqrt(pi) exp(-alpha^2 r^2) / r^2 - erf(alpha r) / r^3.  With ewald_real on
    the same grid: ewald_real.C - ewald_excluded.C = prefactor / r."""
    r = pair_table.knots(r_min, r_max, nknots)
    a = float(alpha)
    e = np.array([math.erf(a * v) for v in r])
    return _out(prefactor, _TWO_OVER_SQRT_PI * a * np.exp(-(a * r) ** 2) / r ** 2 - e / r ** 3, -e / r)


def ewald_self(alpha, charges, prefactor=1.0):
    """The self-energy of Ewald / PME, ``-prefactor alpha / sqrt(pi) sum q_i^2``: a host scalar from a host array of charges."""
    q = np.asarray(charges, dtype=np.float64)
    return -float(prefactor) * float(alpha) / math.sqrt(math.pi) * float((q * q).sum())


def wolf(alpha, r_cut, r_min, r_max, nknots, prefactor=1.0):
    """Wolf's damped, energy-shifted sum: C = erfc(alpha r) / r - erfc(alpha r_cut) / r_cut (its self term
    ``-(erfc(alpha r_cut) / (2 r_cut) + alpha / sqrt(pi)) sum q_i^2`` is a host scalar and the caller's)."""
    r = pair_table.knots(r_min, r_max, nknots)
    c, f = _damped(float(alpha), r)
    c_cut = _damped(float(alpha), np.array([float(r_cut)]))[0][0]
    return _out(prefactor, f / r, c - c_cut)


def dsf(alpha, r_cut, r_min, r_max, nknots, prefactor=1.0):
    """Fennell and Gezelter's damped shifted force: energy and force both vanish at r_cut,
    C = erfc(alpha r) / r - erfc(alpha r_cut) / r_cut + f_cut (r - r_cut), f_cut the damped force at r_cut."""
    r = pair_table.knots(r_min, r_max, nknots)
    c, f = _damped(float(alpha), r)
    c_cut, f_cut = (v[0] for v in _damped(float(alpha), np.array([float(r_cut)])))
    return _out(prefactor, (f - f_cut) / r, c - c_cut + f_cut * (r - float(r_cut)))


def reaction_field(eps_rf, r_cut, r_min, r_max, nknots, prefactor=1.0):
    """A reaction field of dielectric eps_rf beyond r_cut (``math.inf``: conducting): C = 1 / r + k r^2 - c with
    k = (eps_rf - 1) / ((2 eps_rf + 1) r_cut^3) and c = 1 / r_cut + k r_cut^2, so that C(r_cut) = 0."""
    r = pair_table.knots(r_min, r_max, nknots)
    rc = float(r_cut)
    k = (0.5 if math.isinf(eps_rf) else (float(eps_rf) - 1.0) / (2.0 * float(eps_rf) + 1.0)) / rc ** 3
    return _out(prefactor, 1.0 / r ** 3 - 2.0 * k, 1.0 / r + k * r * r - (1.0 / rc + k * rc * rc))


def debye(kappa, r_min, r_max, nknots, prefactor=1.0):
    """Debye-Hueckel screened Coulomb: C = exp(-kappa r) / r."""
    r = pair_table.knots(r_min, r_max, nknots)
    e = np.exp(-float(kappa) * r)
    return _out(prefactor, e * (float(kappa) * r + 1.0) / r ** 3, e / r)


def shifted(r_cut, r_min, r_max, nknots, prefactor=1.0):
    """Plain Coulomb shifted to zero at r_cut: C = 1 / r - 1 / r_cut."""
    r = pair_table.knots(r_min, r_max, nknots)
    return _out(prefactor, 1.0 / r ** 3, 1.0 / r - 1.0 / float(r_cut))


def interpolate(K, C, r_min, r_max, r2):
    """``(kc, cc, in)`` of the rule of nl_set_coulomb_table in float64 for an array of r^2: pair_table.interpolate on the charge
    table.  The pair's force over r is ``q_i q_j kc``, its energy ``q_i q_j cc``; NaN below r_min^2, 0 outside ``in``."""
    return pair_table.interpolate(K, C, r_min, r_max, r2)

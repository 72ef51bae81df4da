"""Steinhardt bond-orientational order parameters, host side of nl_set_steinhardt (include/nl_hip.h).

numpy only: importable without the HIP library.
``wigner3j_table(l)`` makes the table of 3j symbols (l l l; m1 m2 m3) that the w_l columns need, by the Racah formula in exact
rational arithmetic, rounded to double once.  ``CRYSTALS`` holds q4, q6, w4, w6 of ideal first shells (Steinhardt, Nelson and
Ronchetti 1983), ``classify`` picks the nearest of them.
"""
from __future__ import annotations

import decimal
import functools
from fractions import Fraction
from math import factorial

import numpy as np

MAX_L = 12  # NL_STEIN_MAX_L


def _wigner3j_squared(l, m1, m2, m3):
    """(sign, value^2) of (l l l; m1 m2 m3) as an int and a Fraction (Racah's formula)."""
    if m1 + m2 + m3 != 0 or max(abs(m1), abs(m2), abs(m3)) > l:
        return 0, Fraction(0)
    tri = Fraction(factorial(l) ** 3, factorial(3 * l + 1))
    pre = tri * factorial(l + m1) * factorial(l - m1) * factorial(l + m2) * factorial(l - m2) * factorial(l + m3) * factorial(l - m3)
    total = Fraction(0)
    for k in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
        den = factorial(k) * factorial(l - k) * factorial(l - m1 - k) * factorial(l + m2 - k) * factorial(m1 + k) * factorial(k - m2)
        total += Fraction((-1) ** k, den)
    sign = (1 if total > 0 else -1 if total < 0 else 0) * (-1) ** (m3 % 2)  # (-1)^(j1 - j2 - m3) with j1 = j2
    return sign, pre * total * total


def _sqrt_to_double(v):
    """sqrt of a non-negative Fraction, rounded to double once (60 digits in between)."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float((decimal.Decimal(v.numerator) / decimal.Decimal(v.denominator)).sqrt())


@functools.lru_cache(maxsize=None)
def _table(l):
    w = np.zeros((2 * l + 1, 2 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            sign, sq = _wigner3j_squared(l, m1, m2, -m1 - m2)
            if sign:
                w[m1 + l, m2 + l] = sign * _sqrt_to_double(sq)
    w.setflags(write=False)
    return w


def wigner3j_table(l):
    """``(2 l + 1, 2 l + 1)`` float64: ``[m1 + l][m2 + l] = (l l l; m1 m2 -m1-m2)``, 0 where ``|m1 + m2| > l`` -- the w3j_host
    of nl_set_steinhardt.  Exact rational arithmetic up to one square root per entry; stands alone (no sympy)."""
    l = int(l)
    if l < 0:
        raise ValueError("l must be >= 0")
    return _table(l).copy()


# q4, q6, w4, w6 (w normalised) of ideal first shells; "bcc14" is the first and second shell of bcc together
CRYSTALS = {
    "fcc": (0.190941, 0.574524, -0.159317, -0.013161),
    "hcp": (0.097222, 0.484762, +0.134097, -0.012442),
    "bcc": (0.509175, 0.628539, -0.159317, +0.013161),
    "bcc14": (0.036370, 0.510688, +0.159317, +0.013161),
    "sc": (0.763763, 0.353553, +0.159317, +0.013161),
}
# the spread each of the four carries among the shells above: the unit a distance to them is measured in
_SCALE = np.ptp(np.array(list(CRYSTALS.values())), axis=0)


def classify(q4, q6, w4, w6, names=None):
    """The shell of ``CRYSTALS`` (of ``names``) nearest to every particle's (q4, q6, w4, w6), each of the four in units of its
    spread over CRYSTALS: ``(index (n,) int, distance (n,))``, the index into ``names`` (default: all five, in CRYSTALS'
    order); -1 where a value is NaN.  A nearest-prototype rule for inspection, not a calibrated classifier: thermal systems
    want thresholds fitted to their own distributions."""
    names = list(CRYSTALS) if names is None else list(names)
    v = np.stack([np.asarray(a, dtype=np.float64) for a in (q4, q6, w4, w6)], axis=-1)
    proto = np.array([CRYSTALS[k] for k in names])
    d = np.sqrt((((v[..., None, :] - proto) / _SCALE) ** 2).sum(axis=-1))
    bad = np.isnan(d).any(axis=-1)
    idx = np.where(bad, -1, np.argmin(np.where(np.isnan(d), np.inf, d), axis=-1))
    return idx, np.where(bad, np.nan, np.min(np.where(np.isnan(d), np.inf, d), axis=-1))

"""From pair-distance histograms to radial distribution functions (host side of nl_pair_histogram, include/nl_hip.h).

numpy only: importable without the HIP library.  A histogram is ``(nbins,)`` counts of pairs, every pair once, in bins
uniform in r up to r_max; a typed one is ``(nslots, nbins)`` with one row per unordered pair of types, row ``slot(a, b)``.
"""
from __future__ import annotations

import numpy as np


def nslots(ntypes):
    """Unordered pairs of ntypes types."""
    return ntypes * (ntypes + 1) // 2


def slot(a, b, ntypes):
    """Row of the pair of types (a, b) in a typed histogram: a (2 ntypes - a + 1) / 2 + (b - a) with a <= b."""
    a, b = (a, b) if a <= b else (b, a)
    if not 0 <= a <= b < ntypes:
        raise ValueError(f"types ({a}, {b}) outside 0 .. {ntypes - 1}")
    return a * (2 * ntypes - a + 1) // 2 + (b - a)


def expand_slots(hist, ntypes):
    """The symmetric ``(ntypes, ntypes, nbins)`` array of a typed ``(nslots, nbins)`` histogram."""
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[0] != nslots(ntypes):
        raise ValueError(f"a typed histogram of {ntypes} types has {nslots(ntypes)} rows")
    out = np.empty((ntypes, ntypes, hist.shape[1]), dtype=hist.dtype)
    for a in range(ntypes):
        for b in range(a, ntypes):
            out[a, b] = out[b, a] = hist[slot(a, b, ntypes)]
    return out


def shell_volumes(r_max, nbins):
    """V_shell,b = 4 pi / 3 ((b + 1)^3 - b^3) (r_max / nbins)^3."""
    b = np.arange(nbins, dtype=np.float64)
    return 4.0 * np.pi / 3.0 * ((b + 1.0) ** 3 - b ** 3) * (float(r_max) / nbins) ** 3


def rdf(hist, r_max, volume, n_a, n_b=None, frames=1):
    """``(r_mid, g)`` of one histogram row: g_b = hist_b / (frames P V_shell,b / volume), P = n_a (n_a - 1) / 2 for like
    particles (n_b None) and n_a n_b for unlike ones -- the pairs an ideal gas of that density would put into the bin."""
    hist = np.asarray(hist, dtype=np.float64)
    if hist.ndim != 1:
        raise ValueError("rdf takes one (nbins,) row of counts")
    nbins = hist.shape[0]
    pairs = 0.5 * n_a * (n_a - 1) if n_b is None else float(n_a) * float(n_b)
    r_mid = (np.arange(nbins) + 0.5) * (float(r_max) / nbins)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = hist / (frames * pairs * shell_volumes(r_max, nbins) / float(volume))
    return r_mid, g

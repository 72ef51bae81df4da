"""Stillinger-Weber three-body potentials, host side of nl_set_sw (include/nl_hip.h).

numpy only: importable without the HIP library.
E = sum_pairs phi(r) + sum_i sum_{j<k} Lambda (cos theta_jik - c0)^2 g(r_ij) g(r_ik).  The pair part phi is a table of
``pair_table`` (``pair`` gives its callables), the radial function g a table in the same knot format, sampled with
``G = -g'(r) / r`` at ``pair_table.knots(r_min_3, r_max_3, nknots)``, one row ``a ntypes + b`` per centre type a and end type b
(``radial``, ``sample``); ``angular`` makes the ``ntypes^3`` arrays Lambda = lambda epsilon and cos0.  ``three_body`` is the
rule of nl_set_sw in float64 over the ordered pairs of a full list: the tests' reference and a user's inspection tool, as
``pair_table.interpolate`` is.
"""
from __future__ import annotations

import numpy as np

from . import pair_table

MAX_TYPES = 4   # NL_SW_MAX_TYPES
MAX_NEAR = 64   # NL_SW_MAX_NEAR


def pair(A, B, p, q, epsilon, sigma, a):
    """``(u, du_dr)`` of the two-body part, float64 callables for ``pair_table.sample``:
    u = A epsilon (B (sigma / r)^p - (sigma / r)^q) exp(sigma / (r - a sigma)) below a sigma, exactly 0 from there on."""
    rc = a * sigma

    def parts(r):
        r = np.asarray(r, dtype=np.float64)
        inside = r < rc
        rs = np.where(inside, r, 0.5 * rc)
        x = sigma / (rs - rc)
        return inside, rs, x, np.exp(x)

    def u(r):
        inside, rs, _, e = parts(r)
        return np.where(inside, A * epsilon * (B * (sigma / rs) ** p - (sigma / rs) ** q) * e, 0.0)

    def du(r):
        inside, rs, x, e = parts(r)
        poly = B * (sigma / rs) ** p - (sigma / rs) ** q
        dpoly = (-p * B * (sigma / rs) ** p + q * (sigma / rs) ** q) / rs
        return np.where(inside, A * epsilon * e * (dpoly - poly * x * x / sigma), 0.0)

    return u, du


def radial(gamma, sigma, a):
    """``(g, dg_dr)`` of the radial factor of the three-body part: g = exp(gamma sigma / (r - a sigma)) below a sigma; g and g'
    are exactly 0 from ``r >= a sigma`` on."""
    rc = a * sigma

    def parts(r):
        r = np.asarray(r, dtype=np.float64)
        inside = r < rc
        rs = np.where(inside, r, 0.5 * rc)
        return inside, rs, np.exp(gamma * sigma / (rs - rc))

    def g(r):
        inside, _, e = parts(r)
        return np.where(inside, e, 0.0)

    def dg(r):
        inside, rs, e = parts(r)
        return np.where(inside, -e * gamma * sigma / (rs - rc) ** 2, 0.0)

    return g, dg


def sample(g, dg_dr, r_min_3, r_max_3, nknots):
    """``(g, G)`` for nl_set_sw from float64 callables g(r) and dg_dr(r) = g'(r): g and ``G = -g'(r) / r`` at the knots.  One
    callable each: arrays of ``(nknots,)``; ntypes x ntypes nested sequences ``[a][b]`` (centre a, end b): ``(ntypes^2, nknots)``."""
    r = pair_table.knots(r_min_3, r_max_3, nknots)
    if callable(g):
        return np.asarray(g(r), dtype=np.float64) + 0.0 * r, -np.asarray(dg_dr(r), dtype=np.float64) / r
    nt = len(g)
    if any(len(row) != nt for row in g) or len(dg_dr) != nt or any(len(row) != nt for row in dg_dr):
        raise ValueError("g and dg_dr need ntypes x ntypes callables each")
    gv = np.stack([np.asarray(g[a][b](r), dtype=np.float64) + 0.0 * r for a in range(nt) for b in range(nt)])
    G = np.stack([-np.asarray(dg_dr[a][b](r), dtype=np.float64) / r for a in range(nt) for b in range(nt)])
    return gv, G


def angular(lam, epsilon, cos0):
    """``(Lambda, cos0)`` of nl_set_sw, ``(ntypes, ntypes, ntypes)`` float64 each, ``[a][b][c]`` with a the centre:
    Lambda = lam epsilon.  Scalars give one type; arrays must be symmetric in the two ends."""
    L = np.asarray(lam, dtype=np.float64) * np.asarray(epsilon, dtype=np.float64)
    c = np.asarray(cos0, dtype=np.float64)
    L, c = np.broadcast_arrays(L, c)
    if L.ndim == 0:
        L, c = L.reshape(1, 1, 1), c.reshape(1, 1, 1)
    if L.ndim != 3 or len(set(L.shape)) != 1:
        raise ValueError("lam epsilon and cos0 must be scalars or (ntypes, ntypes, ntypes)")
    if not (np.array_equal(L, L.transpose(0, 2, 1)) and np.array_equal(c, c.transpose(0, 2, 1))):
        raise ValueError("Lambda and cos0 must be symmetric in the two ends")
    return np.ascontiguousarray(L), np.ascontiguousarray(c)


def silicon():
    """The parameter set of Stillinger and Weber, Phys. Rev. B 31, 5262 (1985), in eV and Angstrom."""
    return dict(epsilon=2.1683, sigma=2.0951, a=1.80, lam=21.0, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584, p=4.0, q=0.0)


def triples(I, m_of):
    """Every ordered pair (P, K), P != K, of entries with the same centre, for entries sorted by centre: I the centre of every
    entry, m_of the entries per centre.  Returns the two index arrays into the entries."""
    start = np.concatenate([[0], np.cumsum(m_of)])[:-1]
    reps = m_of[I]
    P = np.repeat(np.arange(len(I)), reps)
    first = np.concatenate([[0], np.cumsum(reps)])[:-1]
    K = start[I[P]] + (np.arange(len(P)) - first[P])
    keep = P != K
    return P[keep], K[keep]


def three_body(n, I, J, d, g, G, r_min_3, r_max_3, lam, cos0, types=None, parts=False, max_near=MAX_NEAR):
    """The three-body part of the rule of nl_set_sw in float64 over the entries of a FULL list: I, J the centre and the partner
    of every entry (both directions of every pair), d = r_i - r_j at the image.  g, G: ``(nknots,)`` or ``(ntypes^2, nknots)``;
    lam, cos0: ``angular``'s arrays; types: ``(n,)`` for more than one type.  Returns a dict: ``f[n, 4]`` = {fx, fy, fz, pe_i}
    (a third of h per particle of a triple), ``w[6]`` (xx, yy, zz, xy, xz, yz: -sum a_c F_j,d), ``u`` (every triple once), ``near[n]``
    (partners in_3 of every centre) and ``in3`` (per entry).  A centre with more than max_near partners gives NaN to itself, to
    those partners and to w and u; a partner below r_min_3 gives what the arithmetic gives.  parts: also ``ends`` = (e, a, F_j,
    e_j), e the entries in_3 sorted by centre, and ``tri`` = (P, K, cs, c0, Lambda, ga, gb, Ga, ira, irb) per ordered pair of
    them (indices into e)."""
    I, J, d = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(d, dtype=np.float64)
    g, G = np.atleast_2d(np.asarray(g, dtype=np.float64)), np.atleast_2d(np.asarray(G, dtype=np.float64))
    lam, cos0 = np.asarray(lam, dtype=np.float64), np.asarray(cos0, dtype=np.float64)
    nt = lam.shape[0]
    if g.shape[0] != nt * nt or lam.shape != (nt,) * 3 or cos0.shape != (nt,) * 3 or (nt > 1 and types is None):
        raise ValueError("g, G of ntypes^2 rows, lam and cos0 of (ntypes,) * 3, and types for ntypes > 1")
    ty = np.zeros(n, dtype=np.int64) if nt == 1 else np.asarray(types, dtype=np.int64)
    r2 = (d * d).sum(axis=1)
    in3 = (r2 < float(r_max_3) ** 2) & (r2 > 0)
    e = np.flatnonzero(in3)
    e = e[np.argsort(I[e], kind="stable")]
    Ie, Je, a, r2e = I[e], J[e], d[e], r2[e]
    near = np.bincount(Ie, minlength=n)
    slot = ty[Ie] * nt + ty[Je]
    ga, Ga = np.zeros(len(e)), np.zeros(len(e))
    for s in np.unique(slot):
        msk = slot == s
        Ga[msk], ga[msk], _ = pair_table.interpolate(G[s], g[s], r_min_3, r_max_3, r2e[msk])
    ir = 1.0 / np.sqrt(r2e)
    P, K = triples(Ie, near)
    over = near > max_near
    ok = ~over[Ie[P]]
    P, K = P[ok], K[ok]
    b = a[K]
    L, c0 = lam[ty[Ie[P]], ty[Je[P]], ty[Je[K]]], cos0[ty[Ie[P]], ty[Je[P]], ty[Je[K]]]
    cs = (((a[P, 0] * b[:, 0] + a[P, 1] * b[:, 1]) + a[P, 2] * b[:, 2]) * ir[P]) * ir[K]
    dc = cs - c0
    ld = L * dc
    ldd = ld * dc
    q = ga[P] * ga[K]
    h = ldd * q
    a2 = (ld + ld) * q
    cb = a2 * (ir[P] * ir[K])
    ca = ldd * (Ga[P] * ga[K]) + a2 * (cs * (ir[P] * ir[P]))
    m = len(e)
    sa, ej = np.bincount(P, weights=ca, minlength=m), np.bincount(P, weights=h, minlength=m)
    sb = np.stack([np.bincount(P, weights=cb * b[:, c], minlength=m) for c in range(3)], axis=1)
    Fj = sb - sa[:, None] * a
    f = np.zeros((n, 4))
    for c in range(3):
        f[:, c] = np.bincount(Je, weights=Fj[:, c], minlength=n) - np.bincount(Ie, weights=Fj[:, c], minlength=n)
    f[:, 3] = np.bincount(Je, weights=ej, minlength=n) / 3.0 + np.bincount(Ie, weights=ej, minlength=n) / 6.0
    ab = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    w = np.array([-(a[:, c] * Fj[:, dd]).sum() for c, dd in ab])
    u = 0.5 * ej.sum()
    if over.any():
        f[over] = np.nan
        f[Je[over[Ie]]] = np.nan
        w[:], u = np.nan, np.nan
    out = dict(f=f, w=w, u=u, near=near, in3=in3)
    if parts:
        out["ends"] = (e, a, Fj, ej)
        out["tri"] = (P, K, cs, c0, L, ga[P], ga[K], Ga[P], ir[P], ir[K])
    return out

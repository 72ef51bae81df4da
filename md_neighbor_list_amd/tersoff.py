"""Tersoff-type bond-order potentials, host side of nl_set_tersoff (include/nl_hip.h).

numpy only: importable without the HIP library.
E = sum_pairs phi(r) + sum_i sum_{j != i} 1/2 b(zeta_ij) u(r_ij), zeta_ij = p(r_ij) sum_{k != i, j} g(cos theta_jik) q(r_ik).
For Tersoff phi = f_C A exp(-lambda_1 r) (``repulsive``, a table of ``pair_table``), u = -f_C B exp(-lambda_2 r) (``attractive``),
q = f_C exp(-lambda_3 r) and p = exp(lambda_3 r) (``zeta_radial``; the m = 1 form), f_C the LAMMPS cut-off function (``cutoff``).
``sample`` makes the knot arrays of the radial tables, ``angular`` and ``bond_order`` the parameter arrays.  ``bond_energy`` is
the rule of nl_set_tersoff in float64 over the ordered pairs of a full list: the tests' reference and a user's inspection tool,
as ``sw.three_body`` is.
"""
from __future__ import annotations

import numpy as np

from . import pair_table, sw

MAX_TYPES = 4   # NL_TERSOFF_MAX_TYPES
MAX_NEAR = 64   # NL_TERSOFF_MAX_NEAR


def cutoff(R, D):
    """``(fc, dfc_dr)``, float64 callables: the LAMMPS f_C, 1 below R - D, 1/2 - 1/2 sin(pi/2 (r - R) / D) to R + D, exactly 0
    from there on."""
    def fc(r):
        r = np.asarray(r, dtype=np.float64)
        x = np.clip((r - R) / D, -1.0, 1.0)
        return np.where(r < R - D, 1.0, np.where(r < R + D, 0.5 - 0.5 * np.sin(0.5 * np.pi * x), 0.0))

    def dfc(r):
        r = np.asarray(r, dtype=np.float64)
        x = np.clip((r - R) / D, -1.0, 1.0)
        return np.where((r > R - D) & (r < R + D), -(0.25 * np.pi / D) * np.cos(0.5 * np.pi * x), 0.0)

    return fc, dfc


def _cut_exp(amp, lam, R, D):
    """(f, df) of amp f_C(r) exp(-lam r)."""
    fc, dfc = cutoff(R, D)

    def f(r):
        r = np.asarray(r, dtype=np.float64)
        return amp * fc(r) * np.exp(-lam * r)

    def df(r):
        r = np.asarray(r, dtype=np.float64)
        return amp * (dfc(r) - lam * fc(r)) * np.exp(-lam * r)

    return f, df


def repulsive(A, lam1, R, D):
    """``(phi, dphi_dr)`` of the repulsive part f_C A exp(-lambda_1 r), for ``pair_table.sample``."""
    return _cut_exp(A, lam1, R, D)


def attractive(B, lam2, R, D):
    """``(u, du_dr)`` of the attractive part u = -f_C B exp(-lambda_2 r), for ``sample``."""
    return _cut_exp(-B, lam2, R, D)


def zeta_radial(lam3, R, D):
    """``((q, dq_dr), (p, dp_dr))`` of the radial factors of zeta: q = f_C exp(-lambda_3 r) and p = exp(lambda_3 r).  With
    lambda_3 = 0 the caller leaves p out of nl_set_tersoff."""
    def p(r):
        return np.exp(lam3 * np.asarray(r, dtype=np.float64))

    def dp(r):
        return lam3 * np.exp(lam3 * np.asarray(r, dtype=np.float64))

    return _cut_exp(1.0, lam3, R, D), (p, dp)


def sample(f, df_dr, r_min_3, r_max_3, nknots):
    """``(f, F)`` for nl_set_tersoff from float64 callables f(r) and df_dr(r): f and ``F = -f'(r) / r`` at the knots.  One
    callable each: arrays of ``(nknots,)``; ntypes x ntypes nested sequences ``[a][b]`` (centre a, end b): ``(ntypes^2, nknots)``."""
    return sw.sample(f, df_dr, r_min_3, r_max_3, nknots)


def angular(gamma, c, d, h):
    """``(gamma, c2_over_d2, d2, h)`` of nl_set_tersoff, ``(ntypes, ntypes, ntypes)`` float64 each, ``[a][b][c]`` with a the
    centre, from the LAMMPS parameters gamma, c, d, h = cos theta_0.  Scalars give one type."""
    g, c, d, h = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (gamma, c, d, h)))
    if g.ndim == 0:
        g, c, d, h = (v.reshape(1, 1, 1) for v in (g, c, d, h))
    if g.ndim != 3 or len(set(g.shape)) != 1:
        raise ValueError("gamma, c, d, h must be scalars or (ntypes, ntypes, ntypes)")
    if not np.all(d != 0):
        raise ValueError("d must not be 0")
    return tuple(np.ascontiguousarray(v) for v in (g + 0.0, (c * c) / (d * d), d * d, h + 0.0))


def bond_order(beta, n):
    """``(beta, n)`` of nl_set_tersoff, ``(ntypes, ntypes)`` float64 each, ``[a][b]`` centre and end.  Scalars give one type."""
    b, n = np.broadcast_arrays(np.asarray(beta, dtype=np.float64), np.asarray(n, dtype=np.float64))
    if b.ndim == 0:
        b, n = b.reshape(1, 1), n.reshape(1, 1)
    if b.ndim != 2 or b.shape[0] != b.shape[1]:
        raise ValueError("beta and n must be scalars or (ntypes, ntypes)")
    if not (np.all(b >= 0) and np.all(n > 0)):
        raise ValueError("beta >= 0 and n > 0")
    return np.ascontiguousarray(b + 0.0), np.ascontiguousarray(n + 0.0)


def silicon():
    """The Si(C) set of Tersoff, Phys. Rev. B 38, 9902 (1988), in eV and Angstrom (the LAMMPS Si.tersoff file)."""
    return dict(A=1830.8, B=471.18, lam1=2.4799, lam2=1.7322, beta=1.1e-6, n=0.78734, c=100390.0, d=16.217, h=-0.59825, R=2.85, D=0.15,
                gamma=1.0, lam3=0.0)


def g_of(cs, gamma, c2_over_d2, d2, h):
    """``(g, dg_dcs)`` of the rule's rearranged angular function in float64."""
    gc = gamma * c2_over_d2
    x = h - cs
    x2 = x * x
    den = d2 + x2
    return gamma + gc * (x2 / den), -(((gc + gc) * d2) * x) / (den * den)


def b_of(zeta, beta, n):
    """``(b, db_dzeta)`` of the rule's bond order in float64: 1 and 0 for zeta <= 0; a NaN zeta propagates."""
    zeta = np.asarray(zeta, dtype=np.float64)
    flat = zeta <= 0
    z = np.where(flat, 1.0, zeta)
    with np.errstate(invalid="ignore", over="ignore"):
        tn = (beta * z) ** n
        b = (1.0 + tn) ** (-1.0 / (2.0 * n))
        bp = ((-0.5 * b) * (tn / (1.0 + tn))) / z
    return np.where(flat, 1.0, b), np.where(flat, 0.0, bp)


def bond_energy(n, I, J, d, u, U, q, Q, r_min_3, r_max_3, gamma, c2_over_d2, d2, h, beta, nn, p=None, P=None, types=None, parts=False,
                max_near=MAX_NEAR):
    """The bond-order part of the rule of nl_set_tersoff in float64 over the entries of a FULL list: I, J the centre and the
    partner of every entry (both directions of every pair), d = r_i - r_j at the image.  u, U, q, Q (p, P): ``(nknots,)`` or
    ``(ntypes^2, nknots)``; gamma, c2_over_d2, d2, h: ``angular``'s arrays; beta, nn: ``bond_order``'s; types: ``(n,)`` for more
    than one type.  Returns a dict: ``f[n, 4]`` = {fx, fy, fz, pe_i} (a quarter of b u per end of every ordered bond), ``w[6]``
    (xx, yy, zz, xy, xz, yz: -sum a_c F_j,d), ``u`` (sum of b u / 2), ``near[n]`` (partners in_3 of every centre) and ``in3`` (per
    entry).  A centre with more than max_near partners gives NaN to itself, to those partners and to w and u; a partner below
    r_min_3 gives what the arithmetic gives.  parts: also ``ends`` = (e, a, F_j, e_j), e the entries in_3 sorted by centre,
    ``bond`` = a dict of per-end arrays (u, U, q, Q, p, P, S, zeta, b, bp, w, ir, beta, n) and ``tri`` = a dict of arrays per
    ordered pair of ends (P, K: indices into e; cs, g_jk, gp_jk, g_kj, gp_kj, and jk, kj: the four parameters of each)."""
    I, J, d = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64), np.asarray(d, dtype=np.float64)
    tabs = [np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (u, U, q, Q)]
    has_p = p is not None
    if has_p:
        tabs += [np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (p, P)]
    ang = [np.asarray(v, dtype=np.float64) for v in (gamma, c2_over_d2, d2, h)]
    beta, nn = np.asarray(beta, dtype=np.float64), np.asarray(nn, dtype=np.float64)
    nt = ang[0].shape[0]
    if tabs[0].shape[0] != nt * nt or any(a.shape != (nt,) * 3 for a in ang) or beta.shape != (nt, nt) or nn.shape != (nt, nt) or \
            (nt > 1 and types is None):
        raise ValueError("tables of ntypes^2 rows, angular arrays of (ntypes,) * 3, beta and n of (ntypes,) * 2, and types for ntypes > 1")
    ty = np.zeros(n, dtype=np.int64) if nt == 1 else np.asarray(types, dtype=np.int64)
    r2 = (d * d).sum(axis=1)
    in3 = (r2 < float(r_max_3) ** 2) & (r2 > 0)
    e = np.flatnonzero(in3)
    e = e[np.argsort(I[e], kind="stable")]
    Ie, Je, a, r2e = I[e], J[e], d[e], r2[e]
    m = len(e)
    near = np.bincount(Ie, minlength=n)
    slot = ty[Ie] * nt + ty[Je]
    uj, Uj, qj, Qj = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    pj, Pj = np.ones(m), np.zeros(m)
    for s in np.unique(slot):
        msk = slot == s
        Uj[msk], uj[msk], _ = pair_table.interpolate(tabs[1][s], tabs[0][s], r_min_3, r_max_3, r2e[msk])
        Qj[msk], qj[msk], _ = pair_table.interpolate(tabs[3][s], tabs[2][s], r_min_3, r_max_3, r2e[msk])
        if has_p:
            Pj[msk], pj[msk], _ = pair_table.interpolate(tabs[5][s], tabs[4][s], r_min_3, r_max_3, r2e[msk])
    ir = 1.0 / np.sqrt(r2e)
    Pi, K = sw.triples(Ie, near)
    over = near > max_near
    ok = ~over[Ie[Pi]]
    Pi, K = Pi[ok], K[ok]
    bv = a[K]
    ti, tj, tk = ty[Ie[Pi]], ty[Je[Pi]], ty[Je[K]]
    jk = [v[ti, tj, tk] for v in ang]
    kj = [v[ti, tk, tj] for v in ang]
    cs = (((a[Pi, 0] * bv[:, 0] + a[Pi, 1] * bv[:, 1]) + a[Pi, 2] * bv[:, 2]) * ir[Pi]) * ir[K]
    g_jk, gp_jk = g_of(cs, *jk)
    g_kj, gp_kj = g_of(cs, *kj)
    S = np.bincount(Pi, weights=g_jk * qj[K], minlength=m)
    zeta = pj * S
    be, ne = beta[ty[Ie], ty[Je]], nn[ty[Ie], ty[Je]]
    b, bp = b_of(zeta, be, ne)
    ej = b * uj
    w = (0.5 * uj) * bp
    wp = w * pj
    cc = (wp[Pi] * gp_jk) * qj[K] + (wp[K] * gp_kj) * qj[Pi]
    cb = cc * (ir[Pi] * ir[K])
    ca = cc * (cs * (ir[Pi] * ir[Pi])) + (wp[K] * g_kj) * Qj[Pi]
    sa = np.bincount(Pi, weights=ca, minlength=m)
    sb = np.stack([np.bincount(Pi, weights=cb * bv[:, c], minlength=m) for c in range(3)], axis=1)
    rad = (0.5 * b) * Uj + (w * Pj) * S
    Fj = sb - (sa + rad)[:, None] * a
    f = np.zeros((n, 4))
    for c in range(3):
        f[:, c] = np.bincount(Je, weights=Fj[:, c], minlength=n) - np.bincount(Ie, weights=Fj[:, c], minlength=n)
    f[:, 3] = (np.bincount(Je, weights=ej, minlength=n) + np.bincount(Ie, weights=ej, minlength=n)) / 4.0
    ab = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    wv = np.array([-(a[:, c] * Fj[:, dd]).sum() for c, dd in ab])
    ut = 0.5 * ej.sum()
    if over.any():
        f[over] = np.nan
        f[Je[over[Ie]]] = np.nan
        wv[:], ut = np.nan, np.nan
    out = dict(f=f, w=wv, u=ut, near=near, in3=in3)
    if parts:
        out["ends"] = (e, a, Fj, ej)
        out["bond"] = dict(u=uj, U=Uj, q=qj, Q=Qj, p=pj, P=Pj, S=S, zeta=zeta, b=b, bp=bp, w=w, ir=ir, beta=be, n=ne)
        out["tri"] = dict(P=Pi, K=K, cs=cs, g_jk=g_jk, gp_jk=gp_jk, g_kj=g_kj, gp_kj=gp_kj, jk=jk, kj=kj)
    return out

"""What tests/test_pair_table.py checks the tabulated pair potentials against (nl_set_pair_table): an
O(N^2) float64 sum of md_neighbor_list_amd.pair_table.interpolate on the caller's double tables, a numpy emulation of the
kernel's arithmetic in the position type, and the potentials the tests tabulate.  No list is used, the library's or the
oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S defined here."""
import numpy as np

from md_neighbor_list_amd import pair_table, rdf
from tests.util import emulate_pairs, lj_pairs
from tests.virial_util import _AB, _row_sums

# 4 x the largest ratio of test_pair_table.test_emulation_gives_c: forces and energies per particle (fp32 emulation), and the
# 7 totals (emulated in fp32 and fp64: their double sums are the whole error of an fp64 list)
TABLE_C = 10.7
TABLE_CW = 1.95


# ------------------------------------------------------------------------------------------------------- potentials
def morse(De=1.0, a=1.5, r0=1.125):
    """(u, du_dr) of U = De ((1 - exp(-a (r - r0)))^2 - 1): at r = 2.5 still -0.24 De, with a slope of 0.33 De."""
    def u(r):
        e = np.exp(-a * (r - r0))
        return De * ((1.0 - e) ** 2 - 1.0)

    def du(r):
        e = np.exp(-a * (r - r0))
        return 2.0 * De * a * (1.0 - e) * e

    return u, du


def lj(eps=1.0, sig=1.0):
    """(u, du_dr) of plain Lennard-Jones, neither shifted nor switched."""
    def u(r):
        s6 = (sig / r) ** 6
        return 4.0 * eps * (s6 * s6 - s6)

    def du(r):
        s6 = (sig / r) ** 6
        return -24.0 * eps * (2.0 * s6 * s6 - s6) / r

    return u, du


def lj_u_xx(x, eps=1.0, sig=1.0):
    """d^2 U / dx^2 of U(x) = 4 eps (sig^12 x^-6 - sig^6 x^-3), x = r^2."""
    return 4.0 * eps * (42.0 * sig ** 12 * x ** -8.0 - 12.0 * sig ** 6 * x ** -5.0)


def lj_f_xx(x, eps=1.0, sig=1.0):
    """d^2 F / dx^2 of F(x) = 24 eps (2 sig^12 x^-7 - sig^6 x^-4), x = r^2: what bounds the interpolation error of an LJ table,
    |F_table - F| <= D^2 max |F_xx| / 8 on a segment."""
    return 24.0 * eps * (112.0 * sig ** 12 * x ** -9.0 - 20.0 * sig ** 6 * x ** -6.0)


# -------------------------------------------------------------------------------------------------------- reference
def _slots(types, ntypes, I, J):
    if ntypes == 1:
        return np.zeros(len(I), dtype=np.int64)
    a, b = np.minimum(types[I], types[J]), np.maximum(types[I], types[J])
    return a * (2 * ntypes - a + 1) // 2 + (b - a)


def table_pairs(q, F, U, r_min, r_max, pairs, types=None, rc_ab=None):
    """Per ordered pair of `pairs` that the list holds and that lies within r_max: (I, J, d, fr, pe, mf, mu) in float64 --
    pair_table.interpolate on the pair's slot and the uncancelled magnitudes |F_k| + |F_k+1| + |dF_k| r2 / D (likewise for
    U): the third term is the conditioning of s = (r2 - x0) / D on the rounding of r2.  rc_ab: the type table's cut-offs; a pair
    of types with rc_ab = 0 is not in the list."""
    F, U = np.atleast_2d(np.asarray(F, dtype=np.float64)), np.atleast_2d(np.asarray(U, dtype=np.float64))
    nslots, nk = F.shape
    nt = int(round(((8 * nslots + 1) ** 0.5 - 1) / 2))
    assert rdf.nslots(nt) == nslots and (nt == 1 or types is not None)
    types = None if types is None else np.asarray(types, dtype=np.int64)
    I, J, d, _ = pairs
    r2 = (d * d).sum(axis=1)
    keep = (r2 > 0) & (r2 < float(r_max) ** 2)
    if rc_ab is not None:
        keep &= np.asarray(rc_ab)[types[I], types[J]] > 0
    I, J, d, r2 = I[keep], J[keep], d[keep], r2[keep]
    sl = _slots(types, nt, I, J)
    D = pair_table.spacing(r_min, r_max, nk)
    fr, pe, mf, mu = (np.zeros(len(I)) for _ in range(4))
    for s in range(nslots):
        m = sl == s
        fr[m], pe[m], inn = pair_table.interpolate(F[s], U[s], r_min, r_max, r2[m])
        assert inn.all()
        k = np.clip(((r2[m] - float(r_min) ** 2) / D).astype(np.int64), 0, nk - 2)
        for tab, out in ((F[s], mf), (U[s], mu)):
            out[m] = np.abs(tab[k]) + np.abs(tab[k + 1]) + np.abs(tab[k + 1] - tab[k]) * r2[m] / D
    return I, J, d, fr, pe, mf, mu


def table_reference(q, box6, mask, F, U, r_min, r_max, pairs=None, types=None, rc_ab=None):
    """Forces and per-particle energies of the table by an O(N^2) float64 sum: (want[n, 4], S[n, 4]), the layout of
    tests.util lj_reference.  pairs: lj_pairs(q, box6, mask, >= r_max) to reuse."""
    n = len(q)
    pairs = lj_pairs(q, box6, mask, float(r_max)) if pairs is None else pairs
    I, _, d, fr, pe, mf, mu = table_pairs(q, F, U, r_min, r_max, pairs, types, rc_ab)
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fr * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=mf * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=0.5 * pe, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n)
    return want, S


def table_virial_reference(q, box6, mask, F, U, r_min, r_max, pairs=None, types=None, rc_ab=None):
    """The 8 totals of the table: (want[8], S[7]), the layout of tests.virial_util virial_reference; every unordered pair
    once (1/2 per ordered pair)."""
    n = len(q)
    pairs = lj_pairs(q, box6, mask, float(r_max)) if pairs is None else pairs
    I, J, d, fr, pe, mf, mu = table_pairs(q, F, U, r_min, r_max, pairs, types, rc_ab)
    # Summed in long double: u S of these sums is only a few ulp of the float64 result itself (S / |W| is about 6), so a
    # float64 sum over 10^5 terms would spend the fp64 bound on the reference's own rounding.
    assert np.finfo(np.longdouble).nmant >= 63, "table_virial_reference needs an extended-precision long double"
    fl, pl, dl = fr.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    n_in = np.nan if np.isnan(fr).any() else 0.5 * len(I)  # (a pair below the table: all 8 are NaN)
    want = np.array([float(0.5 * (fl * dl[:, a] * dl[:, b]).sum()) for a, b in _AB] + [float(0.5 * pl.sum()), n_in])
    S = np.array([0.5 * (mf * np.abs(d[:, a] * d[:, b])).sum() for a, b in _AB] + [0.5 * mu.sum()])
    return want, S


# -------------------------------------------------------------------------------------------------------- emulation
def table_device_form(F, U, r_min, r_max, T):
    """The knots {F, dF, U, dU} and the scalars x0, xc, iD in T, as nl_set_pair_table makes them from the double tables."""
    T = np.dtype(T).type
    F, U = np.atleast_2d(np.asarray(F, dtype=np.float64)), np.atleast_2d(np.asarray(U, dtype=np.float64))
    z = np.zeros((F.shape[0], 1))
    dF, dU = np.concatenate([np.diff(F, axis=1), z], axis=1), np.concatenate([np.diff(U, axis=1), z], axis=1)
    D = pair_table.spacing(r_min, r_max, F.shape[1])
    return tuple(v.astype(T) for v in (F, dF, U, dU)) + (T(float(r_min) ** 2), T(float(r_max) ** 2), T(1.0 / D))


def _knot(r2, x0, xc, iD, nk, T):
    """table_knot of csrc/nl_table.inc in T: (in, below, k, t)."""
    inn = (r2 < xc) & (r2 > 0)
    below = r2 < x0
    s = (r2 - x0) * iD
    ok = inn & ~below
    k = np.where(ok, np.minimum(np.where(ok, s, T(0)).astype(np.int32), nk - 2), 0)
    return inn, below, k, s - k.astype(T)


def _lin(V, dV, sl, k, t, inn, below, T):
    """table_read of csrc/nl_table.inc in T, on the knots k of the slots sl."""
    return np.where(inn, np.where(below, T(np.nan), V[sl, k] + t * dV[sl, k]), T(0))


def _sum_rows(n, I, term, rng):
    """Per particle the sum in term's type of its rows of term[m, c], every particle's terms in a random order (tests.util
    lj_emulate's sum)."""
    order = np.lexsort((rng.random(len(I)), I))
    Is, term = I[order], term[order]
    rank = np.arange(len(Is)) - np.searchsorted(Is, np.arange(n))[Is]
    out = np.zeros((n, term.shape[1]), dtype=term.dtype)
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        out[Is[sel]] += term[sel]
    return out


def _block_sum(v, nblk=1):
    """block_sum of csrc/nl_virial.inc on a grid of nblk blocks of 256 threads, in double: thread g of the grid adds v[g],
    v[g + 256 nblk], ... in that order, then a tree over the threads of each block.  Returns the nblk sums."""
    acc = np.zeros(nblk * 256)
    for i0 in range(0, len(v), nblk * 256):
        chunk = v[i0:i0 + nblk * 256]
        acc[:len(chunk)] += chunk
    acc = acc.reshape(nblk, 256)
    while acc.shape[1] > 1:
        acc = acc[:, :acc.shape[1] // 2] + acc[:, acc.shape[1] // 2:]
    return acc[:, 0]


def table_emulate_pairs(q, box6, mask, F, U, r_min, r_max, T, pairs, types=None, knot_shift=0, use_t=True):
    """lj_image (tests.util emulate_pairs) and TableByPair::pair (csrc/nl_table.inc) in the position type T over the ordered
    pairs (I, J): one rounding per operation, no FMA.  Returns (dx, dy, dz, fx, fy, fz, pe, in) in T.  knot_shift, use_t: the
    deliberate defects of test_wrong_results_are_rejected (a neighbouring knot; t ignored)."""
    T = np.dtype(T).type
    I, J = pairs[0], pairs[1]
    dx, dy, dz = emulate_pairs(q, box6, mask, 1.0, 1.0, 1.0, T, pairs)[:3]
    Ft, dFt, Ut, dUt, x0, xc, iD = table_device_form(F, U, r_min, r_max, T)
    nslots, nk = Ft.shape
    nt = int(round(((8 * nslots + 1) ** 0.5 - 1) / 2))
    sl = _slots(None if types is None else np.asarray(types, dtype=np.int64), nt, I, J)
    inn, below, k, t = _knot(dx * dx + dy * dy + dz * dz, x0, xc, iD, nk, T)
    k = np.clip(k + knot_shift, 0, nk - 2)
    if not use_t:
        t = np.zeros_like(t)
    fr, pe = _lin(Ft, dFt, sl, k, t, inn, below, T), _lin(Ut, dUt, sl, k, t, inn, below, T)
    out = (dx, dy, dz, fr * dx, fr * dy, fr * dz, pe, inn)
    assert all(v.dtype == np.dtype(T) for v in out[:7])
    return out


def table_emulate(q, box6, mask, F, U, r_min, r_max, T, rng, pairs, types=None, **defect):
    """The row body of k_table_forces over table_emulate_pairs' values, f = {fx, fy, fz, pe / 2} summed per particle in T
    (_sum_rows).  Returns f[n, 4] in T."""
    T = np.dtype(T).type
    _, _, _, fx, fy, fz, pe, _ = table_emulate_pairs(q, box6, mask, F, U, r_min, r_max, T, pairs, types=types, **defect)
    term = np.stack([fx, fy, fz, T(0.5) * pe], axis=1)
    assert term.dtype == np.dtype(T)
    return _sum_rows(len(q), pairs[0], term, rng)


def table_virial_emulate(n, I, vals, rng, nblk=512):
    """k_table_virial and k_virial_reduce over table_emulate_pairs' values of the ordered pairs of a FULL list, with the
    kernels' own summation tree: the six products and the energy in T, converted to double; row i goes to wave i mod 4 nblk,
    its entries (in a random order) to the lanes in turn, every lane adds its terms one after the other; then the butterfly
    of the wave, waves ((0 + 1) + 2) + 3, the partials of the blocks by _block_sum, and the factor 1/2 of a full list.
    Returns the 7 sums and n_in."""
    dx, dy, dz, fx, fy, fz, pe, inn = vals
    terms = [fx * dx, fy * dy, fz * dz, fx * dy, fx * dz, fy * dz, pe]
    assert all(t.dtype == dx.dtype for t in terms)
    nblk = min((n + 3) // 4, nblk)
    order = np.lexsort((rng.random(len(I)), I))
    Is = I[order]
    pos = np.arange(len(Is)) - np.searchsorted(Is, np.arange(n))[Is]  # the entry's place in its row
    wave, lane = Is % (4 * nblk), pos % 64
    key = np.lexsort((pos // 64, Is // (4 * nblk), lane, wave))  # a lane's terms in the order it meets them
    out = np.zeros(7)
    for c, t in enumerate(terms):
        acc = np.bincount((wave * 64 + lane)[key], weights=t.astype(np.float64)[order][key], minlength=4 * nblk * 64)  # (adds in order)
        acc = acc.reshape(nblk, 4, 64)
        while acc.shape[2] > 1:  # wave_sum
            acc = acc[:, :, :acc.shape[2] // 2] + acc[:, :, acc.shape[2] // 2:]
        part = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
        out[c] = 0.5 * _block_sum(part)[0]
    return np.concatenate([out, [0.5 * inn.sum()]])

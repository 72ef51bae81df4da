"""What tests/test_sw.py checks the Stillinger-Weber calls against (nl_set_sw): a float64 evaluation of
the rule of include/nl_hip.h through md_neighbor_list_amd.sw three_body and pair_table.interpolate on the caller's double tables
over an O(N^2) pair sweep, a numpy emulation of the rule in the position type, and the potential the tests tabulate.  No list
is used, the library's or the oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S defined
here."""
import numpy as np

from md_neighbor_list_amd import sw
from tests.util import emulate_pairs
from tests.util_eam import _read
from tests.util_table import _block_sum, _knot, _lin, _slots, _sum_rows, table_device_form
from tests.virial_util import _AB

# 4 x the largest ratios of test_sw.test_emulation_gives_c, each the larger of the fp32 and the fp64 emulation: forces and
# energies per particle and column (0.509: the energies, fp64; fp32 0.456; the force components 0.145), and the 7 totals (0.0634:
# U, fp64; the virial 0.048; fp32 0.036)
SW_C = 2.04
SW_CW = 0.254

A_SIGMA = 3.2  # where the test g would vanish: beyond every table's end, so g(r_max_3) is 0.18 and a dropped partner shows


# -------------------------------------------------------------------------------------------------------- potential
def sw_functions(nt):
    """(g, dg_dr), nt x nt callables each: the Stillinger-Weber radial form exp(gamma_ab / (r - A_SIGMA)) with
    gamma_ab = 1.2 + 0.15 a - 0.1 b, which is not symmetric in (a, b): at r = 2.5 between 0.13 and 0.21, at r = 1 about 0.55."""
    gs, dgs = [], []
    for a in range(nt):
        row = [sw.radial(1.2 + 0.15 * a - 0.1 * b, 1.0, A_SIGMA) for b in range(nt)]
        gs.append([r[0] for r in row]), dgs.append([r[1] for r in row])
    return gs, dgs


def sw_angular(nt):
    """(Lambda, cos0) of (nt,) * 3: different for every triple of types, symmetric in the two ends."""
    a, b, c = np.meshgrid(*(np.arange(nt, dtype=np.float64),) * 3, indexing="ij")
    lam = 1.0 + 0.3 * a + 0.1 * (b + c) + 0.05 * b * c
    cos0 = -1.0 / 3.0 + 0.1 * a - 0.04 * (b + c) + 0.02 * b * c
    return sw.angular(lam, 1.0, cos0)


class SwTables:
    """The double tables of one potential: the pair table (F, U) on (r_min, r_max), the radial tables (g, G) on
    (r_min_3, r_max_3), every array 2-d with one row per slot, and the angular parameters lam, cos0 of (nt,) * 3."""

    def __init__(self, F, U, r_min, r_max, g, G, r_min_3, r_max_3, lam, cos0):
        self.F, self.U, self.g, self.G = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (F, U, g, G))
        self.lam, self.cos0 = sw.angular(lam, 1.0, cos0)
        self.r_min, self.r_max, self.r_min_3, self.r_max_3 = (float(v) for v in (r_min, r_max, r_min_3, r_max_3))
        self.nt = self.lam.shape[0]
        self.nt_pair = int(round(((8 * self.F.shape[0] + 1) ** 0.5 - 1) / 2))
        assert self.g.shape[0] == self.nt ** 2 and self.nt_pair in (1, self.nt)

    @property
    def reach(self):
        return max(self.r_max, self.r_max_3)


# -------------------------------------------------------------------------------------------------------- reference
def sw_list_pairs(tab, pairs, types=None, rc_ab=None, exclusions=None, n=None):
    """(I, J, d, r2) of the entries a full list holds within the reach of the tables: a pair of types with rc_ab = 0, or an
    excluded pair, is not in the list."""
    I, J, d, _ = pairs
    r2 = (d * d).sum(axis=1)
    keep = (r2 > 0) & (r2 < tab.reach ** 2)
    if rc_ab is not None:
        keep &= np.asarray(rc_ab)[types[I], types[J]] > 0
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keep &= ~np.isin(I * n + J, np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]]))
    return I[keep], J[keep], d[keep], r2[keep]


def sw_reference(q, box6, mask, tab, pairs, types=None, rc_ab=None, exclusions=None):
    """The rule of nl_set_sw in float64: a dict of want[n, 4] = {fx, fy, fz, pe_i} and S[n, 4], the totals ww[8] and SW[7], the
    partners in_3 per centre near[n], and the list's entries.  S: the uncancelled sums over pairs (the three terms of a table
    read, section 8o) and over triples, built with |cs| + |c0| in place of |dc| and the table-read magnitudes of g and G, which
    carry the conditioning of each read on the rounding of its r2."""
    n = len(q)
    types = None if types is None else np.asarray(types, dtype=np.int64)
    assert tab.nt == 1 or types is not None
    I, J, d, r2 = sw_list_pairs(tab, pairs, types, rc_ab, exclusions, n)
    frp, pe, mf, mu, in_p = _read(tab.F, tab.U, tab.r_min, tab.r_max, _slots(types, tab.nt_pair, I, J), r2)
    tb = sw.three_body(n, I, J, d, tab.g, tab.G, tab.r_min_3, tab.r_max_3, tab.lam, tab.cos0, types=types, parts=True)
    e, a, Fj, ej = tb["ends"]
    P, K, cs, c0, L, _, _, _, ira, irb = tb["tri"]
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    Ie, Je = I[e], J[e]
    _, _, mG, mg, _ = _read(tab.G, tab.g, tab.r_min_3, tab.r_max_3, ty[Ie] * tab.nt + ty[Je], r2[e])
    DC, aL, b = np.abs(cs) + np.abs(c0), np.abs(L), a[K]
    Mh = aL * DC * DC * mg[P] * mg[K]
    Ma2 = 2.0 * aL * DC * mg[P] * mg[K]
    Mcb, Mca = Ma2 * ira * irb, aL * DC * DC * mG[P] * mg[K] + Ma2 * np.abs(cs) * ira * ira
    m = len(e)
    SF = np.stack([np.bincount(P, weights=Mcb * np.abs(b[:, c]) + Mca * np.abs(a[P, c]), minlength=m) for c in range(3)], axis=1)
    Sh = np.bincount(P, weights=Mh, minlength=m)
    want, S = tb["f"].copy(), np.zeros((n, 4))
    for c in range(3):
        want[:, c] += np.bincount(I, weights=frp * d[:, c], minlength=n)
        S[:, c] = np.bincount(I, weights=mf * np.abs(d[:, c]), minlength=n) + np.bincount(Je, weights=SF[:, c], minlength=n) + \
            np.bincount(Ie, weights=SF[:, c], minlength=n)
    want[:, 3] += np.bincount(I, weights=0.5 * pe, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n) + np.bincount(Je, weights=Sh, minlength=n) / 3.0 + np.bincount(Ie, weights=Sh, minlength=n) / 6.0
    assert np.finfo(np.longdouble).nmant >= 63, "sw_reference needs an extended-precision long double"
    fl, pl, dl = frp.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    al, Fl = a.astype(np.longdouble), Fj.astype(np.longdouble)
    ww = np.array([float(0.5 * (fl * dl[:, c] * dl[:, dd]).sum() - (al[:, c] * Fl[:, dd]).sum()) for c, dd in _AB] +
                  [float(0.5 * pl.sum() + 0.5 * ej.astype(np.longdouble).sum()), 0.5 * (in_p | tb["in3"]).sum()])
    if np.isnan(want).any() or np.isnan(ww).any():
        ww[:] = np.nan
    SW = np.array([0.5 * (mf * np.abs(d[:, c] * d[:, dd])).sum() + (np.abs(a[:, c]) * SF[:, dd]).sum() for c, dd in _AB] +
                  [0.5 * mu.sum() + 0.5 * Sh.sum()])
    return dict(want=want, S=S, ww=ww, SW=SW, near=tb["near"], entries=(I, J, d, r2), three=tb["f"], triples=len(P) // 2)


def sw_energy(q, box6, mask, fns, r_max, r_max_3, lam, cos0, pairs):
    """E of the ANALYTIC one-type potential fns = (u, g) truncated at r_max and r_max_3, in float64: what the gradient test
    differentiates.  pairs: lj_pairs of q."""
    u, g = fns
    I, J, d, _ = pairs
    r = np.sqrt((d * d).sum(axis=1))
    E = 0.5 * u(r[r < r_max]).sum()
    e = np.flatnonzero(r < r_max_3)
    e = e[np.argsort(I[e], kind="stable")]
    P, K = sw.triples(I[e], np.bincount(I[e], minlength=len(q)))
    a, b, ra, rb = d[e][P], d[e][K], r[e][P], r[e][K]
    cs = (a * b).sum(axis=1) / (ra * rb)
    return E + 0.5 * (lam * (cs - cos0) ** 2 * g(ra) * g(rb)).sum()


# -------------------------------------------------------------------------------------------------------- emulation
DEFECTS = ("a dropped triple", "G_b for G_a", "the slot (t_j, t_i)", "Lambda of a permuted triple", "no third of h for an end",
           "no -cs a ir_a^2", "a triple twice in U")


def _virial_tree(n, I, pos, pair_terms, e, lane3, three_terms, nblk=512):
    """The summation tree of k_sw_virial and k_virial_reduce in double: row i goes to wave i mod 4 nblk; an entry at place pos of
    its row adds its pair term in lane pos mod 64, chunk after chunk; behind them the row's compacted partner lane3 adds its
    three-body term; every lane keeps its sum across its rows; then the butterfly of the wave, waves ((0 + 1) + 2) + 3, the
    partials of the blocks by _block_sum, and the factor 1/2 of a full list."""
    nblk = min((n + 3) // 4, nblk)
    rows = np.concatenate([I, I[e]])
    lane = np.concatenate([pos % 64, lane3])
    stage = np.concatenate([pos // 64, np.full(len(e), 1 << 30)])
    wave, gen = rows % (4 * nblk), rows // (4 * nblk)
    key = np.lexsort((stage, gen, lane, wave))
    out = np.zeros(len(pair_terms))
    for c, (tp, t3) in enumerate(zip(pair_terms, three_terms)):
        v = np.concatenate([tp.astype(np.float64), t3.astype(np.float64)])
        acc = np.bincount((wave * 64 + lane)[key], weights=v[key], minlength=4 * nblk * 64).reshape(nblk, 4, 64)  # (adds in order)
        while acc.shape[2] > 1:
            acc = acc[:, :, :acc.shape[2] // 2] + acc[:, :, acc.shape[2] // 2:]
        part = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
        out[c] = 0.5 * _block_sum(part)[0]
    return out


def sw_emulate(q, box6, mask, tab, T, rng, entries, types=None, defect=None, totals=True):
    """The rule of nl_set_sw in the position type T over the entries (I, J) of a FULL list, as csrc/nl_sw.inc walks it: lj_image
    (tests.util emulate_pairs), the pair table's read, in_3, the per-partner and the per-ordered-pair operations in the order the
    header gives, one rounding per operation, no FMA, knots and scalars rounded as the setters round them; sa, sb, e_j, the
    centre's sums and every particle's atomics each summed in a random order; the totals with the kernels' own tree over a random
    order of every row.  Returns f[n, 4] in T and w[8].  defect: one of DEFECTS."""
    T = np.dtype(T).type
    n, I, J = len(q), entries[0], entries[1]
    types = None if types is None else np.asarray(types, dtype=np.int64)
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    nt = tab.nt
    dx, dy, dz = emulate_pairs(q, box6, mask, 1.0, 1.0, 1.0, T, entries)[:3]
    r2 = dx * dx + dy * dy + dz * dz
    Ft, dFt, Ut, dUt, x0, xc, iD = table_device_form(tab.F, tab.U, tab.r_min, tab.r_max, T)
    Gt, dGt, gt, dgt, x03, xc3, iD3 = table_device_form(tab.G, tab.g, tab.r_min_3, tab.r_max_3, T)
    lam, cos0 = tab.lam.astype(T), tab.cos0.astype(T)
    in_p, below_p, kp, tp = _knot(r2, x0, xc, iD, Ft.shape[1], T)
    sl = _slots(types, tab.nt_pair, I, J)
    frp, pe = _lin(Ft, dFt, sl, kp, tp, in_p, below_p, T), _lin(Ut, dUt, sl, kp, tp, in_p, below_p, T)
    fx, fy, fz = frp * dx, frp * dy, frp * dz
    in3 = (r2 < xc3) & (r2 > 0)
    # the row order of the list is not the reference's: a random one, which is also the order of the compaction
    order = np.lexsort((rng.random(len(I)), I))
    pos = np.empty(len(I), dtype=np.int64)
    pos[order] = np.arange(len(I)) - np.searchsorted(I[order], np.arange(n))[I[order]]
    e = order[in3[order]]
    Ie, Je = I[e], J[e]
    near = np.bincount(Ie, minlength=n)
    assert near.max() <= sw.MAX_NEAR, "sw_emulate has no overflow path"
    lane3 = np.arange(len(e)) - np.searchsorted(Ie, np.arange(n))[Ie]
    ax, ay, az, r2e = dx[e], dy[e], dz[e], r2[e]
    in_e, below_e, ke, te = _knot(r2e, x03, xc3, iD3, gt.shape[1], T)
    slot = ty[Je] * nt + ty[Ie] if defect == "the slot (t_j, t_i)" else ty[Ie] * nt + ty[Je]
    ga, Ga = _lin(gt, dgt, slot, ke, te, in_e, below_e, T), _lin(Gt, dGt, slot, ke, te, in_e, below_e, T)
    ir = T(1) / np.sqrt(r2e)
    ir2 = ir * ir
    P, K = sw.triples(Ie, near)
    ti, tj, tk = ty[Ie[P]], ty[Je[P]], ty[Je[K]]
    L, c0 = (lam[tj, ti, tk] if defect == "Lambda of a permuted triple" else lam[ti, tj, tk]), cos0[ti, tj, tk]
    bx, by, bz = ax[K], ay[K], az[K]
    cs = (((ax[P] * bx + ay[P] * by) + az[P] * bz) * ir[P]) * ir[K]
    dc = cs - c0
    ld = L * dc
    ldd = ld * dc
    qq = ga[P] * ga[K]
    h = ldd * qq
    a2 = (ld + ld) * qq
    cb = a2 * (ir[P] * ir[K])
    ca = ldd * ((Ga[K] if defect == "G_b for G_a" else Ga[P]) * ga[K])
    if defect != "no -cs a ir_a^2":
        ca = ca + a2 * (cs * ir2[P])
    term = np.stack([ca, cb * bx, cb * by, cb * bz, h], axis=1)
    assert term.dtype == np.dtype(T)
    if defect == "a dropped triple":  # an ordinary one: the median |h| of all triples, from both its ends
        k = int(np.argsort(np.abs(h))[len(h) // 2])
        term = term[~(((P == P[k]) & (K == K[k])) | ((P == K[k]) & (K == P[k])))]
        P = P[~(((P == P[k]) & (K == K[k])) | ((P == K[k]) & (K == P[k])))]
    s = _sum_rows(len(e), P, term, rng)
    Fj = np.stack([s[:, 1] - s[:, 0] * ax, s[:, 2] - s[:, 0] * ay, s[:, 3] - s[:, 0] * az], axis=1)
    ej = s[:, 4]
    own = _sum_rows(n, I, np.stack([fx, fy, fz, T(0.5) * pe], axis=1), rng)
    centre = _sum_rows(n, Ie, np.concatenate([Fj, ej[:, None]], axis=1), rng)
    own = own + np.concatenate([-centre[:, :3], (centre[:, 3] * T(1.0 / 6.0))[:, None]], axis=1)
    third = np.zeros_like(ej) if defect == "no third of h for an end" else ej * T(1.0 / 3.0)
    f = _sum_rows(n, np.concatenate([np.arange(n), Je]), np.concatenate([own, np.concatenate([Fj, third[:, None]], axis=1)]), rng)
    assert f.dtype == np.dtype(T) and Fj.dtype == np.dtype(T)
    w = None
    if totals:
        av = (ax, ay, az)
        three = [T(-1) * (av[c] * Fj[:, dd]) for c, dd in _AB]
        assert all(t.dtype == np.dtype(T) for t in three)
        three = [2.0 * t.astype(np.float64) for t in three] + [(2.0 if defect == "a triple twice in U" else 1.0) * ej.astype(np.float64)]
        pair_terms = [fx * dx, fy * dy, fz * dz, fx * dy, fx * dz, fy * dz, pe]
        w = np.concatenate([_virial_tree(n, I, pos, pair_terms, e, lane3, three), [0.5 * (in_p | in3).sum()]])
    return f, w

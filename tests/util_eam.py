"""What tests/test_eam.py checks the embedded-atom calls against (nl_set_eam): an O(N^2) float64
evaluation of the rule of include/nl_hip.h through md_neighbor_list_amd.eam density / embed and pair_table.interpolate on the
caller's double tables, a numpy emulation of the three passes in the position type, and the potential the tests tabulate.
No list is used, the library's or the oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S
defined here."""
import numpy as np

from md_neighbor_list_amd import eam, pair_table
from tests.util import emulate_pairs, lj_pairs
from tests.util_table import _block_sum, _knot, _lin, _slots, _sum_rows, table_device_form, table_virial_emulate
from tests.virial_util import _AB

# 4 x the largest ratios of test_eam.test_emulation_gives_c, every one the larger of the fp32 and the fp64 emulation: forces and
# energies per particle (1.82: the energies; the force components 0.49), the densities (2.35, fp64; fp32 1.76), and the 7 totals
# (0.391: U, fp64)
EAM_C = 7.28
EAM_C_RHO = 9.4
EAM_CW = 1.57

R_E = 1.125      # the lattice spacing of the inputs
RHO_EPS = 1.0    # F(rho) = -C sqrt(rho + RHO_EPS) + D rho^2: regularised, so that F' exists at the first knot, rho = 0


# -------------------------------------------------------------------------------------------------------- potential
def eam_functions(nt):
    """(f, df_dr, F, dF_drho), a list of nt callables each: f_b(r) = A_b exp(-beta_b (r - R_E)), at r = 2.5 still 0.06 A_b with a
    slope of -0.13 A_b, and F_a(rho) = -C_a sqrt(rho + RHO_EPS) + D_a rho^2.  The square root is regularised (RHO_EPS = 1, a
    fifteenth of the densities met) and not cut out at the first knot: the table then samples one smooth function on all of
    [0, rho_max], and the convergence test holds from rho = 0 on."""
    fs, dfs, Fs, dFs = [], [], [], []
    for b in range(nt):
        A, beta, Cc, Dd = 1.0 + 0.25 * b, 2.0 + 0.3 * b, 2.0 + 0.5 * b, 0.005 * (1.0 + 0.4 * b)
        fs.append(lambda r, A=A, beta=beta: A * np.exp(-beta * (r - R_E)))
        dfs.append(lambda r, A=A, beta=beta: -beta * A * np.exp(-beta * (r - R_E)))
        Fs.append(lambda x, Cc=Cc, Dd=Dd: -Cc * np.sqrt(x + RHO_EPS) + Dd * x * x)
        dFs.append(lambda x, Cc=Cc, Dd=Dd: -0.5 * Cc / np.sqrt(x + RHO_EPS) + 2.0 * Dd * x)
    return fs, dfs, Fs, dFs


class EamTables:
    """The double tables of one potential: the pair table (F, U) on (r_min, r_max), the density tables (f, G) on
    (r_min_d, r_max_d), the embedding tables (E, P) on [0, rho_max]; every array 2-d, one row per slot."""

    def __init__(self, F, U, r_min, r_max, f, G, r_min_d, r_max_d, E, P, rho_max):
        self.F, self.U, self.f, self.G, self.E, self.P = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (F, U, f, G, E, P))
        self.r_min, self.r_max, self.r_min_d, self.r_max_d, self.rho_max = (float(v) for v in (r_min, r_max, r_min_d, r_max_d, rho_max))
        self.nt = self.f.shape[0]
        self.nt_pair = int(round(((8 * self.F.shape[0] + 1) ** 0.5 - 1) / 2))
        assert self.E.shape[0] == self.nt and self.nt_pair in (1, self.nt)

    @property
    def reach(self):
        return max(self.r_max, self.r_max_d)

    @property
    def drho(self):
        return self.rho_max / (self.E.shape[1] - 1)


# -------------------------------------------------------------------------------------------------------- reference
def _read(A, B, r_min, r_max, sl, r2):
    """Rows sl of the tables A and B at r2 by pair_table.interpolate: (a, b, ma, mb, in), ma and mb the uncancelled magnitudes
    |A_k| + |A_k+1| + |dA_k| r2 / D of util_table.table_pairs (0 outside in)."""
    nk = A.shape[1]
    D = pair_table.spacing(r_min, r_max, nk)
    a, b, ma, mb = (np.zeros(len(r2)) for _ in range(4))
    inn = np.zeros(len(r2), dtype=bool)
    for s in np.unique(sl):
        m = sl == s
        a[m], b[m], inn[m] = pair_table.interpolate(A[s], B[s], r_min, r_max, r2[m])
        k = np.clip(((r2[m] - r_min ** 2) / D).astype(np.int64), 0, nk - 2)
        for tab, out in ((A[s], ma), (B[s], mb)):
            out[m] = (np.abs(tab[k]) + np.abs(tab[k + 1]) + np.abs(tab[k + 1] - tab[k]) * r2[m] / D) * inn[m]
    return a, b, ma, mb, inn


def _embed_all(tab, ty, rho, S_rho):
    """Per particle (Fe, fp, ME, MP): eam.embed on the particle's slot, and the magnitudes of the two reads -- the three terms of
    a table read, |E_k| + |E_k+1| + |dE_k| rho / Drho, plus the conditioning on the density's own error, |dE_k| / Drho S_rho."""
    n = len(rho)
    Fe, fp, ME, MP = (np.zeros(n) for _ in range(4))
    nk = tab.E.shape[1]
    for a in range(tab.nt):
        m = ty == a
        Fe[m], fp[m] = eam.embed(tab.E[a], tab.P[a], tab.rho_max, rho[m])
        r = np.clip(np.nan_to_num(rho[m]), 0.0, tab.rho_max)
        k = np.minimum((r / tab.drho).astype(np.int64), nk - 2)
        for t, out in ((tab.E[a], ME), (tab.P[a], MP)):
            out[m] = np.abs(t[k]) + np.abs(t[k + 1]) + np.abs(t[k + 1] - t[k]) * (r + S_rho[m]) / tab.drho
    return Fe, fp, ME, MP


def eam_list_pairs(tab, pairs, types=None, rc_ab=None):
    """(I, J, d, r2) of the ordered pairs the list holds within the reach of the tables (rc_ab: a pair of types with rc_ab = 0
    is not in the list)."""
    I, J, d, _ = pairs
    r2 = (d * d).sum(axis=1)
    keep = (r2 > 0) & (r2 < tab.reach ** 2)
    if rc_ab is not None:
        keep &= np.asarray(rc_ab)[types[I], types[J]] > 0
    return I[keep], J[keep], d[keep], r2[keep]


def eam_reference(q, box6, mask, tab, pairs=None, types=None, rc_ab=None, parts=False):
    """The rule of nl_set_eam by an O(N^2) float64 sum: a dict of want[n, 4] = {fx, fy, fz, pe_i} and S[n, 4]; rho[n], S_rho[n],
    fp[n], Fe[n]; the totals ww[8] and SW[7] (summed in long double, as util_table.table_virial_reference).  parts: the pair
    arrays as well (I, J, d, fr, pe, fj, in_d), for the tests that take the sums apart."""
    n = len(q)
    types = None if types is None else np.asarray(types, dtype=np.int64)
    assert tab.nt == 1 or types is not None
    pairs = lj_pairs(q, box6, mask, tab.reach) if pairs is None else pairs
    I, J, d, r2 = eam_list_pairs(tab, pairs, types, rc_ab)
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    frp, pe, mf, mu, in_p = _read(tab.F, tab.U, tab.r_min, tab.r_max, _slots(types, tab.nt_pair, I, J), r2)
    Gj, fj, mGj, mfj, in_d = _read(tab.G, tab.f, tab.r_min_d, tab.r_max_d, ty[J], r2)
    Gi, _, mGi, _, _ = _read(tab.G, tab.f, tab.r_min_d, tab.r_max_d, ty[I], r2)
    rho = np.bincount(I, weights=fj, minlength=n)
    S_rho = np.bincount(I, weights=mfj, minlength=n)
    Fe, fp, ME, MP = _embed_all(tab, ty, rho, S_rho)
    fr = frp + np.where(in_d, fp[I] * Gj + fp[J] * Gi, 0.0)
    mag = mf + MP[I] * mGj + MP[J] * mGi
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fr * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=mag * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=0.5 * pe, minlength=n) + Fe
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n) + ME
    assert np.finfo(np.longdouble).nmant >= 63, "eam_reference needs an extended-precision long double"
    fl, pl, dl = fr.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    bad = np.isnan(fr).any() or np.isnan(Fe).any()
    ww = np.array([float(0.5 * (fl * dl[:, a] * dl[:, b]).sum()) for a, b in _AB] +
                  [float(0.5 * pl.sum() + Fe.astype(np.longdouble).sum()), 0.5 * (in_p | in_d).sum()])
    if bad:
        ww[:] = np.nan
    SW = np.array([0.5 * (mag * np.abs(d[:, a] * d[:, b])).sum() for a, b in _AB] + [0.5 * mu.sum() + ME.sum()])
    out = dict(want=want, S=S, rho=rho, S_rho=S_rho, fp=fp, Fe=Fe, ww=ww, SW=SW)
    if parts:
        out["pairs"] = (I, J, d, fr, pe, fj, in_d)
    return out


def eam_energy(q, box6, mask, fns, r_max, types=None):
    """E of the ANALYTIC potential fns = (u, f[], F[]) truncated at r_max, in float64: what the gradient test differentiates."""
    u, fs, Fs = fns
    n = len(q)
    I, J, d, _ = lj_pairs(q, box6, mask, r_max)
    r = np.sqrt((d * d).sum(axis=1))
    ty = np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    fj = np.zeros(len(r))
    for b in range(len(fs)):
        m = ty[J] == b
        fj[m] = fs[b](r[m])
    rho = np.bincount(I, weights=fj, minlength=n)
    E = 0.5 * u(r).sum()
    for a in range(len(Fs)):
        E += Fs[a](rho[ty == a]).sum()
    return E


# -------------------------------------------------------------------------------------------------------- emulation
def fe_sum_emulate(fe, nblk_max=512):
    """k_eam_fe_part and k_eam_add_u: the Fe_i in double over the grid of k_eam_fe_part, then the partials of its blocks, both by
    util_table._block_sum."""
    return _block_sum(_block_sum(fe.astype(np.float64), min((len(fe) + 255) // 256, nblk_max)))[0]


DEFECTS = ("a pair dropped from the density", "f of the row's type", "fp_i for both ends", "Fe left out", "no reaction in rho")


def eam_emulate(q, box6, mask, tab, T, rng, pairs, types=None, defect=None, totals=True):
    """The three passes of csrc/nl_eam.inc in the position type T over the ordered pairs (I, J) of a FULL list: lj_image
    (tests.util emulate_pairs), EamDensity::pair, k_eam_embed, EamByPair::pair, one rounding per operation, no FMA, knots and
    scalars rounded as the setters round them, every particle's terms summed in a random order; the totals with the kernels'
    own summation tree (util_table.table_virial_emulate, fe_sum_emulate).  Returns (f[n, 4], rho[n]) in T and w[8].
    defect: one of DEFECTS, the deliberate errors of test_wrong_results_are_rejected."""
    T = np.dtype(T).type
    n, I, J = len(q), pairs[0], pairs[1]
    types = None if types is None else np.asarray(types, dtype=np.int64)
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    dx, dy, dz = emulate_pairs(q, box6, mask, 1.0, 1.0, 1.0, T, pairs)[:3]
    r2 = dx * dx + dy * dy + dz * dz
    Ft, dFt, Ut, dUt, x0, xc, iD = table_device_form(tab.F, tab.U, tab.r_min, tab.r_max, T)
    Gt, dGt, ft, dft, x0d, xcd, iDd = table_device_form(tab.G, tab.f, tab.r_min_d, tab.r_max_d, T)
    z = np.zeros((tab.nt, 1))
    Et, dEt, Pt, dPt = (v.astype(T) for v in (tab.E, np.concatenate([np.diff(tab.E, axis=1), z], axis=1), tab.P,
                                              np.concatenate([np.diff(tab.P, axis=1), z], axis=1)))
    iDr, rmax = T(1.0 / tab.drho), T(tab.rho_max)
    # pass 1
    in_d, below_d, kd, td = _knot(r2, x0d, xcd, iDd, ft.shape[1], T)
    src = ty[I] if defect == "f of the row's type" else ty[J]
    fj = _lin(ft, dft, src, kd, td, in_d, below_d, T)
    sel = np.ones(len(I), dtype=bool)
    if defect == "a pair dropped from the density":  # the weakest one: closest to r_max_d, from both its particles
        k = int(np.argmax(np.where(in_d, r2, T(0))))
        sel = ~(((I == I[k]) & (J == J[k])) | ((I == J[k]) & (J == I[k])))
    if defect == "no reaction in rho":  # a half list: every pair reaches the particle of the smaller id only
        sel = I < J
    rho = _sum_rows(n, I[sel], fj[sel, None], rng)[:, 0]
    # pass 2
    ok = (rho >= 0) & (rho <= rmax)
    s = np.where(ok, rho, T(0)) * iDr
    ke = np.minimum(s.astype(np.int32), Et.shape[1] - 2)
    te = s - ke.astype(T)
    nan = T(np.nan)
    Fe, fp = np.where(ok, Et[ty, ke] + te * dEt[ty, ke], nan), np.where(ok, Pt[ty, ke] + te * dPt[ty, ke], nan)
    # pass 3
    in_p, below_p, kp, tp = _knot(r2, x0, xc, iD, Ft.shape[1], T)
    sl = _slots(types, tab.nt_pair, I, J)
    frp, pe = _lin(Ft, dFt, sl, kp, tp, in_p, below_p, T), _lin(Ut, dUt, sl, kp, tp, in_p, below_p, T)
    Gi = np.where(below_d, nan, Gt[ty[I], kd] + td * dGt[ty[I], kd])
    Gj = np.where(below_d, nan, Gt[ty[J], kd] + td * dGt[ty[J], kd])
    fpj = fp[I] if defect == "fp_i for both ends" else fp[J]
    fr = frp + np.where(in_d, fp[I] * Gj + fpj * Gi, T(0))
    fx, fy, fz = fr * dx, fr * dy, fr * dz
    term = np.stack([fx, fy, fz, T(0.5) * pe], axis=1)
    assert term.dtype == np.dtype(T) and rho.dtype == np.dtype(T) and Fe.dtype == np.dtype(T)
    f = _sum_rows(n, I, term, rng)
    if defect != "Fe left out":
        f[:, 3] = f[:, 3] + Fe
    w = None
    if totals:
        w = table_virial_emulate(n, I, (dx, dy, dz, fx, fy, fz, pe, in_p | in_d), rng)
        if defect != "Fe left out":
            w[6] = w[6] + fe_sum_emulate(Fe)
    return f, rho, w

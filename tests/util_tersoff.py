"""What tests/test_tersoff.py checks the Tersoff calls against (nl_set_tersoff): a float64 evaluation of
the rule of include/nl_hip.h through md_neighbor_list_amd.tersoff bond_energy and pair_table.interpolate on the caller's double
tables over an O(N^2) pair sweep, a numpy emulation of the rule in the position type, and the potential the tests tabulate.  No
list is used, the library's or the oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S defined
here."""
import numpy as np

from md_neighbor_list_amd import sw, tersoff
from tests.util import emulate_pairs
from tests.util_eam import _read
from tests.util_sw import _virial_tree
from tests.util_table import _knot, _lin, _slots, _sum_rows, table_device_form
from tests.virial_util import _AB

# 4 x the largest ratios of test_tersoff.test_emulation_gives_c, each the larger of the fp32 and the fp64 emulation: forces and
# energies per particle and column (2.812: the energies, fp64; fp32 2.369; the force components 0.537), and the 7 totals (0.512:
# U, fp64; the virial 0.103; fp32 0.035)
TERSOFF_C = 11.28
TERSOFF_CW = 2.052
POW_ULP = 2  # the accuracy assumed of pow and powf (assumed, not documented)

# the test potential in reduced units: f_C = 1 below 1.0, 0 from 1.9 on -- its ramp holds the first shell of the lattice (1.125,
# jittered between 0.93 and 1.3) and the second (1.59); the third (1.95) and fourth (2.25) are in the list and in the tables,
# where u and q are exactly 0
CUT_R, CUT_D = 1.45, 0.45
R0 = 1.125
Q_DECAY = 4.0


# -------------------------------------------------------------------------------------------------------- potential
def _shifted(amp, lam, R=CUT_R, D=CUT_D):
    """(f, df) of amp f_C(r) exp(-lam (r - R0))."""
    return tersoff._cut_exp(amp * np.exp(lam * R0), lam, R, D)


def tf_functions(nt, lam3=True, R=CUT_R, D=CUT_D):
    """(u, du, q, dq, p, dp), nt x nt callables each, not symmetric in (a, b): u = -f_C B_ab exp(-l2_ab (r - R0)) with
    B_ab = 1 + 0.25 a - 0.15 b, l2_ab = 1.2 + 0.1 a + 0.05 b; q = f_C exp(-l3_ab (r - R0)) exp(-Q_DECAY (r - R0)) and
    p = exp(l3_ab (r - R0)) with l3_ab = 0.4 + 0.15 a - 0.1 b (lam3=False: l3 = 0 and p is None).  The factor
    exp(-Q_DECAY (r - R0)) of q lets the nearest partners dominate zeta, so that the jitter of the lattice spreads it over a
    factor of ten, and b with it."""
    us, dus, qs, dqs, ps, dps = ([] for _ in range(6))
    for a in range(nt):
        row = []
        for b in range(nt):
            l3 = (0.4 + 0.15 * a - 0.1 * b) if lam3 else 0.0
            u = _shifted(-(1.0 + 0.25 * a - 0.15 * b), 1.2 + 0.1 * a + 0.05 * b, R, D)
            q = _shifted(1.0, l3 + Q_DECAY, R, D)
            p = (lambda r, l=l3: np.exp(l * (np.asarray(r, dtype=np.float64) - R0)), lambda r, l=l3: l * np.exp(l * (np.asarray(r, dtype=np.float64) - R0)))
            row.append((u, q, p))
        us.append([r[0][0] for r in row]), dus.append([r[0][1] for r in row])
        qs.append([r[1][0] for r in row]), dqs.append([r[1][1] for r in row])
        ps.append([r[2][0] for r in row]), dps.append([r[2][1] for r in row])
    return us, dus, qs, dqs, (ps if lam3 else None), (dps if lam3 else None)


def tf_repulsive(nt, R=CUT_R, D=CUT_D):
    """(phi, dphi), nt x nt callables each, symmetric: f_C A_ab exp(-l1_ab (r - R0)), A_ab = 0.8 + 0.1 (a + b), l1_ab = 3 + 0.2 a b."""
    rows = [[_shifted(0.8 + 0.1 * (a + b), 3.0 + 0.2 * a * b, R, D) for b in range(nt)] for a in range(nt)]
    return [[f[0] for f in row] for row in rows], [[f[1] for f in row] for row in rows]


def tf_parameters(nt):
    """(gamma, c2_over_d2, d2, h) of (nt,) * 3, different for every triple of types and not symmetric in the ends, and (beta, n) of
    (nt,) * 2, not symmetric: c / d is about 7, so g varies between gamma and about 45 gamma over the angles, with its minimum near
    the right angle of the lattice; beta puts beta zeta between 0.7 and 9, where b bends."""
    a, b, c = np.meshgrid(*(np.arange(nt, dtype=np.float64),) * 3, indexing="ij")
    gamma = 0.02 + 0.005 * a + 0.004 * b - 0.003 * c
    cc = 1.0 + 0.1 * a - 0.05 * b + 0.1 * c
    dd = 0.15 + 0.01 * a + 0.015 * b - 0.01 * c
    hh = 0.0 + 0.1 * a - 0.06 * b + 0.04 * c
    a2, b2 = np.meshgrid(*(np.arange(nt, dtype=np.float64),) * 2, indexing="ij")
    beta = 1.1 * (1.0 + 0.3 * a2 - 0.2 * b2)
    n = 2.5 + 0.4 * a2 - 0.3 * b2
    return tersoff.angular(gamma, cc, dd, hh) + tersoff.bond_order(beta, n)


class TfTables:
    """The double tables of one potential: the pair table (F, U) on (r_min, r_max), the radial tables u, Uu, q, Qq and p, Pp (or
    None) on (r_min_3, r_max_3), every array 2-d with one row per slot, the angular parameters of (nt,) * 3 and beta, n of (nt,) * 2."""

    def __init__(self, F, U, r_min, r_max, u, Uu, q, Qq, p, Pp, r_min_3, r_max_3, gamma, c2d2, d2, h, beta, n):
        two = lambda v: None if v is None else np.atleast_2d(np.asarray(v, dtype=np.float64))  # noqa: E731
        self.F, self.U, self.u, self.Uu, self.q, self.Qq, self.p, self.Pp = (two(v) for v in (F, U, u, Uu, q, Qq, p, Pp))
        self.ang = tuple(np.asarray(v, dtype=np.float64) for v in (gamma, c2d2, d2, h))
        self.nt = self.ang[0].shape[0]
        self.beta, self.n = (np.asarray(v, dtype=np.float64).reshape(self.nt, self.nt) for v in (beta, n))
        self.r_min, self.r_max, self.r_min_3, self.r_max_3 = (float(v) for v in (r_min, r_max, r_min_3, r_max_3))
        self.nt_pair = int(round(((8 * self.F.shape[0] + 1) ** 0.5 - 1) / 2))
        assert self.u.shape[0] == self.nt ** 2 and self.nt_pair in (1, self.nt) and all(a.shape == (self.nt,) * 3 for a in self.ang)

    @property
    def reach(self):
        return max(self.r_max, self.r_max_3)

    def set_args(self):
        """The arguments of NeighListGPU.set_tersoff."""
        return (self.u, self.Uu, self.q, self.Qq, self.r_min_3, self.r_max_3) + self.ang + (self.beta, self.n, self.p, self.Pp)

    def energy_args(self):
        """The arguments of tersoff.bond_energy behind (n, I, J, d)."""
        return (self.u, self.Uu, self.q, self.Qq, self.r_min_3, self.r_max_3) + self.ang + (self.beta, self.n)


# -------------------------------------------------------------------------------------------------------- reference
def tf_list_pairs(tab, pairs, types=None, rc_ab=None, exclusions=None, n=None):
    """(I, J, d, r2) of the entries a full list holds within the reach of the tables (util_sw.sw_list_pairs)."""
    from tests.util_sw import sw_list_pairs

    return sw_list_pairs(tab, pairs, types, rc_ab, exclusions, n)


def _g2(cs, gamma, c2d2, d2, h):
    """|g''| bounded by its uncancelled form: 2 |gc| d2 (den + 4 x^2) / den^3."""
    x2 = (h - cs) ** 2
    den = d2 + x2
    return 2.0 * np.abs(gamma * c2d2) * d2 * (den + 4.0 * x2) / den ** 3


def tf_reference(q, box6, mask, tab, pairs, types=None, rc_ab=None, exclusions=None):
    """The rule of nl_set_tersoff in float64: a dict of want[n, 4] = {fx, fy, fz, pe_i} and S[n, 4], the totals ww[8] and SW[7],
    the partners in_3 per centre near[n], the list's entries, and b, g of every bond and ordered pair of ends.
    S, the uncancelled sums.  Pairs: the three terms of a table read (section 8o).  Bonds: a first-order propagation -- every
    quantity v carries E(v) >= |v|, its own rounding and what it inherits: E(x y) = E(x) |y| + |x| E(y), E(x + y) = E(x) + E(y),
    E(f(x)) = |f| + |f'| E(x).  From the bottom up --
      E of a table read: the three terms;  Ecs = (|ax bx| + |ay by| + |az bz|) ir_a ir_b;  Ex = |h| + Ecs, which stands for the error
      of x = h - cs and does not vanish where x does;
      Eg = |gamma| + |gc| x2 / den + |g'| Ex;   Egp = |g'| + 2 |gc| d2 (den + 4 x2) / den^3 Ex  (|g''| by parts);
      ES = sum_k (Eg |q_k| + |g| Eq_k);   Ezeta = Ep sum_k |g q_k| + |p| ES;
      Eb = b (1 + s / (2 n)) + |b'| Ezeta, s = tn / (1 + tn): the two pow and the conditioning of b on zeta;
      Ebp = |b'| (2 + s / (2 n)) + (|b'| s / (2 zeta) + b s (n (1 - s) + 1) / (2 zeta^2)) Ezeta: likewise for b', |b''| by parts;
      Ee = Eb |u| + b Eu;   Ew = (Eu |b'| + |u| Ebp) / 2;   Ewp = Ew |p| + |w| Ep;
      c1 = wp_j g'_jk q_k and c2 = wp_k g'_kj q_j by the product rule, Ecc = Ec1 + Ec2, Vcc = |c1| + |c2|;
      Ecb = Ecc ir_a ir_b;   Eca = Ecc |cs| ir2_a + Vcc Ecs ir2_a + E(wp_k g_kj Q_j);   Erad = E(b U) / 2 + E(w P S);
      SF_j,c = sum_k (Ecb |b_c| + Eca |a_c|) + Erad |a_c|."""
    n = len(q)
    types = None if types is None else np.asarray(types, dtype=np.int64)
    assert tab.nt == 1 or types is not None
    I, J, d, r2 = tf_list_pairs(tab, pairs, types, rc_ab, exclusions, n)
    frp, pe, mf, mu, in_p = _read(tab.F, tab.U, tab.r_min, tab.r_max, _slots(types, tab.nt_pair, I, J), r2)
    kw = {} if tab.p is None else dict(p=tab.p, P=tab.Pp)
    tb = tersoff.bond_energy(n, I, J, d, *tab.energy_args(), types=types, parts=True, **kw)
    e, a, Fj, ej = tb["ends"]
    B, t3 = tb["bond"], tb["tri"]
    P, K, cs = t3["P"], t3["K"], t3["cs"]
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    Ie, Je = I[e], J[e]
    m = len(e)
    sl = ty[Ie] * tab.nt + ty[Je]
    _, _, MU, Mu, _ = _read(tab.Uu, tab.u, tab.r_min_3, tab.r_max_3, sl, r2[e])
    _, _, MQ, Mq, _ = _read(tab.Qq, tab.q, tab.r_min_3, tab.r_max_3, sl, r2[e])
    if tab.p is None:
        MP, Mp = np.zeros(m), np.ones(m)
    else:
        _, _, MP, Mp, _ = _read(tab.Pp, tab.p, tab.r_min_3, tab.r_max_3, sl, r2[e])
    ir = B["ir"]
    b_ = a[K]
    Ecs = (np.abs(a[P] * b_).sum(axis=1)) * ir[P] * ir[K]
    au, aU, aq, aQ, ap, aP = (np.abs(B[k]) for k in ("u", "U", "q", "Q", "p", "P"))

    def mags(par, g, gp):
        gamma, c2d2, d2, h = par
        Ex = np.abs(h) + Ecs
        x2 = (h - cs) ** 2
        den = d2 + x2
        return np.abs(gamma) + np.abs(gamma * c2d2) * x2 / den + np.abs(gp) * Ex, np.abs(gp) + _g2(cs, *par) * Ex

    g_jk, gp_jk, g_kj, gp_kj = (np.abs(t3[k]) for k in ("g_jk", "gp_jk", "g_kj", "gp_kj"))
    Eg_jk, Egp_jk = mags(t3["jk"], g_jk, gp_jk)
    Eg_kj, Egp_kj = mags(t3["kj"], g_kj, gp_kj)
    ES = np.bincount(P, weights=Eg_jk * aq[K] + g_jk * Mq[K], minlength=m)
    VS = np.bincount(P, weights=g_jk * aq[K], minlength=m)
    Ez = Mp * VS + ap * ES
    zeta, bb, bp, nn_ = B["zeta"], np.abs(B["b"]), np.abs(B["bp"]), B["n"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos = zeta > 0
        zs = np.where(pos, zeta, 1.0)
        tn = np.where(pos, (B["beta"] * zs) ** nn_, 0.0)
        s = tn / (1.0 + tn)
        Eb = bb * (1.0 + s / (2.0 * nn_)) + bp * Ez
        Ebp = bp * (2.0 + s / (2.0 * nn_)) + np.where(pos, bp * s / (2.0 * zs) + bb * s * (nn_ * (1.0 - s) + 1.0) / (2.0 * zs * zs), 0.0) * Ez
    Me = Eb * au + bb * Mu
    aw = 0.5 * au * bp
    Ew = 0.5 * (Mu * bp + au * Ebp)
    awp, Ewp = aw * ap, Ew * ap + aw * Mp
    Ecc = (Ewp[P] * gp_jk * aq[K] + awp[P] * Egp_jk * aq[K] + awp[P] * gp_jk * Mq[K]) + \
        (Ewp[K] * gp_kj * aq[P] + awp[K] * Egp_kj * aq[P] + awp[K] * gp_kj * Mq[P])
    Vcc = awp[P] * gp_jk * aq[K] + awp[K] * gp_kj * aq[P]
    Ecb = Ecc * ir[P] * ir[K]
    Eca = (Ecc * np.abs(cs) + Vcc * Ecs) * ir[P] * ir[P] + (Ewp[K] * g_kj * aQ[P] + awp[K] * Eg_kj * aQ[P] + awp[K] * g_kj * MQ[P])
    Erad = 0.5 * (Eb * aU + bb * MU) + (Ew * aP * VS + aw * MP * VS + aw * aP * ES)
    SF = np.stack([np.bincount(P, weights=Ecb * np.abs(b_[:, c]) + Eca * np.abs(a[P, c]), minlength=m) + Erad * np.abs(a[:, c]) for c in range(3)], axis=1)
    want, S = tb["f"].copy(), np.zeros((n, 4))
    for c in range(3):
        want[:, c] += np.bincount(I, weights=frp * d[:, c], minlength=n)
        S[:, c] = np.bincount(I, weights=mf * np.abs(d[:, c]), minlength=n) + np.bincount(Je, weights=SF[:, c], minlength=n) + \
            np.bincount(Ie, weights=SF[:, c], minlength=n)
    want[:, 3] += np.bincount(I, weights=0.5 * pe, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n) + (np.bincount(Je, weights=Me, minlength=n) + np.bincount(Ie, weights=Me, minlength=n)) / 4.0
    assert np.finfo(np.longdouble).nmant >= 63, "tf_reference needs an extended-precision long double"
    fl, pl, dl = frp.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    al, Fl = a.astype(np.longdouble), Fj.astype(np.longdouble)
    ww = np.array([float(0.5 * (fl * dl[:, c] * dl[:, dd]).sum() - (al[:, c] * Fl[:, dd]).sum()) for c, dd in _AB] +
                  [float(0.5 * pl.sum() + 0.5 * ej.astype(np.longdouble).sum()), 0.5 * (in_p | tb["in3"]).sum()])
    if np.isnan(want).any() or np.isnan(ww).any():
        ww[:] = np.nan
    SW = np.array([0.5 * (mf * np.abs(d[:, c] * d[:, dd])).sum() + (np.abs(a[:, c]) * SF[:, dd]).sum() for c, dd in _AB] +
                  [0.5 * mu.sum() + 0.5 * Me.sum()])
    S, SW = np.nan_to_num(S, nan=0.0, posinf=0.0), np.nan_to_num(SW, nan=0.0, posinf=0.0)  # (where the reference is NaN no bound is looked at)
    return dict(want=want, S=S, ww=ww, SW=SW, near=tb["near"], entries=(I, J, d, r2), bond=tb["f"], b=B["b"], zeta=zeta, g=t3["g_jk"],
                ordered=len(P), ends=(Ie, Je, ej))


def tf_energy(q, fns, par, r_max_3, pairs, types):
    """E of the ANALYTIC potential fns = (phi, u, qf, pf), nested [a][b] callables (phi by unordered pair), with the parameters
    par = (gamma, c2_over_d2, d2, h, beta, n), in float64 and in the textbook form: what the gradient test differentiates.  The
    functions vanish before r_max_3."""
    phi, u, qf, pf = fns
    gamma, c2d2, d2, h, beta, nn = par
    I, J, d, _ = pairs
    r = np.sqrt((d * d).sum(axis=1))
    keep = r < r_max_3
    I, J, d, r = I[keep], J[keep], d[keep], r[keep]
    order = np.argsort(I, kind="stable")
    I, J, d, r = I[order], J[order], d[order], r[order]
    ti, tj = types[I], types[J]
    nt = gamma.shape[0]

    def val(f):
        out = np.zeros(len(r))
        for a in range(nt):
            for b in range(nt):
                msk = (ti == a) & (tj == b)
                out[msk] = f[a][b](r[msk])
        return out

    E = 0.5 * val(phi).sum()
    uv, qv, pv = val(u), val(qf), val(pf)
    P, K = sw.triples(I, np.bincount(I, minlength=len(q)))
    cs = (d[P] * d[K]).sum(axis=1) / (r[P] * r[K])
    a, b, c = ti[P], tj[P], tj[K]
    g = gamma[a, b, c] * (1.0 + c2d2[a, b, c] - c2d2[a, b, c] * d2[a, b, c] / (d2[a, b, c] + (h[a, b, c] - cs) ** 2))
    zeta = pv * np.bincount(P, weights=g * qv[K], minlength=len(I))
    be, ne = beta[ti, tj], nn[ti, tj]
    bo = (1.0 + (be * zeta) ** ne) ** (-1.0 / (2.0 * ne))
    return E + 0.5 * (bo * uv).sum()


# -------------------------------------------------------------------------------------------------------- emulation
DEFECTS = ("a dropped partner in S_j", "g_kj for g_jk", "the slot (t_j, t_i)", "no w_k term", "no P_j term", "b' with the wrong sign",
           "a bond twice in U", "pe quarters misplaced")


def _pow(x, y, T, rng, ulp):
    """numpy's power in T, perturbed at random by up to ulp units in the last place: the model of pow / powf."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.power(x, y)
    assert v.dtype == np.dtype(T)
    if ulp:
        v = v + rng.integers(-ulp, ulp + 1, size=v.shape).astype(T) * np.spacing(np.abs(v))
    return v.astype(T)


def tf_emulate(q, box6, mask, tab, T, rng, entries, types=None, defect=None, totals=True, ulp=POW_ULP):
    """The rule of nl_set_tersoff in the position type T over the entries (I, J) of a FULL list, as csrc/nl_tersoff.inc walks it:
    lj_image (tests.util emulate_pairs), the pair table's read, in_3, the per-partner operations and the two passes in the order
    the header gives, one rounding per operation, no FMA, knots and scalars rounded as the setter rounds them; the two pow by
    _pow; S_j, sa, sb, the centre's sums and every particle's atomics each summed in a random order; the totals with the
    kernels' own tree over a random order of every row.  Returns f[n, 4] in T and w[8].  defect: one of DEFECTS."""
    T = np.dtype(T).type
    n, I, J = len(q), entries[0], entries[1]
    types = None if types is None else np.asarray(types, dtype=np.int64)
    ty = np.zeros(n, dtype=np.int64) if tab.nt == 1 else types
    nt = tab.nt
    dx, dy, dz = emulate_pairs(q, box6, mask, 1.0, 1.0, 1.0, T, entries)[:3]
    r2 = dx * dx + dy * dy + dz * dz
    Ft, dFt, Ut, dUt, x0, xc, iD = table_device_form(tab.F, tab.U, tab.r_min, tab.r_max, T)
    UUt, dUUt, ut, dut, x03, xc3, iD3 = table_device_form(tab.Uu, tab.u, tab.r_min_3, tab.r_max_3, T)
    QQt, dQQt, qt, dqt = table_device_form(tab.Qq, tab.q, tab.r_min_3, tab.r_max_3, T)[:4]
    gamma, c2d2, d2, hh = tab.ang
    gam, gc, d2, hh = gamma.astype(T), (gamma * c2d2).astype(T), d2.astype(T), hh.astype(T)
    beta, nn, e2 = tab.beta.astype(T), tab.n.astype(T), (-1.0 / (2.0 * tab.n)).astype(T)
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
    assert near.max() <= tersoff.MAX_NEAR, "tf_emulate has no overflow path"
    lane3 = np.arange(len(e)) - np.searchsorted(Ie, np.arange(n))[Ie]
    ax, ay, az, r2e = dx[e], dy[e], dz[e], r2[e]
    in_e, below_e, ke, te = _knot(r2e, x03, xc3, iD3, ut.shape[1], T)
    slot = ty[Je] * nt + ty[Ie] if defect == "the slot (t_j, t_i)" else ty[Ie] * nt + ty[Je]
    uj, Uj = _lin(ut, dut, slot, ke, te, in_e, below_e, T), _lin(UUt, dUUt, slot, ke, te, in_e, below_e, T)
    qj, Qj = _lin(qt, dqt, slot, ke, te, in_e, below_e, T), _lin(QQt, dQQt, slot, ke, te, in_e, below_e, T)
    if tab.p is None:
        pj, Pj = np.ones(len(e), dtype=T), np.zeros(len(e), dtype=T)
    else:
        PPt, dPPt, pt, dpt = table_device_form(tab.Pp, tab.p, tab.r_min_3, tab.r_max_3, T)[:4]
        pj, Pj = _lin(pt, dpt, slot, ke, te, in_e, below_e, T), _lin(PPt, dPPt, slot, ke, te, in_e, below_e, T)
    ir = T(1) / np.sqrt(r2e)
    ir2 = ir * ir
    P, K = sw.triples(Ie, near)
    ti, tj, tk = ty[Ie[P]], ty[Je[P]], ty[Je[K]]
    bx, by, bz = ax[K], ay[K], az[K]
    cs = (((ax[P] * bx + ay[P] * by) + az[P] * bz) * ir[P]) * ir[K]

    def g_of(a, b, c):
        x = hh[a, b, c] - cs
        x2 = x * x
        den = d2[a, b, c] + x2
        return gam[a, b, c] + gc[a, b, c] * (x2 / den), -((((gc[a, b, c] + gc[a, b, c]) * d2[a, b, c]) * x) / (den * den))

    g_jk, gp_jk = g_of(ti, tj, tk)
    g_kj, gp_kj = g_of(ti, tk, tj)
    first = (g_kj if defect == "g_kj for g_jk" else g_jk) * qj[K]
    assert first.dtype == np.dtype(T)
    keep = np.ones(len(P), dtype=bool)
    if defect == "a dropped partner in S_j":  # an ordinary one: the median of the terms that are not 0 (beyond f_C they are)
        live = np.flatnonzero(first != 0)
        keep[int(live[np.argsort(np.abs(first[live]))[len(live) // 2]])] = False
    m = len(e)
    S = _sum_rows(m, P[keep], first[keep, None], rng)[:, 0]
    zeta = pj * S
    be, ne, ee = beta[ty[Ie], ty[Je]], nn[ty[Ie], ty[Je]], e2[ty[Ie], ty[Je]]
    flat = zeta <= 0
    zs = np.where(flat, T(1), zeta)
    t = be * zs
    tn = _pow(t, ne, T, rng, ulp)
    one = T(1) + tn
    b = np.where(flat, T(1), _pow(one, ee, T, rng, ulp))
    bp = np.where(flat, T(0), ((T(-0.5) * b) * (tn / one)) / zs)
    if defect == "b' with the wrong sign":
        bp = -bp
    ej = b * uj
    w = (T(0.5) * uj) * bp
    wp = w * pj
    c2 = (wp[K] * gp_kj) * qj[P]
    third = (wp[K] * g_kj) * Qj[P]
    if defect == "no w_k term":
        c2, third = np.zeros_like(c2), np.zeros_like(third)
    cc = (wp[P] * gp_jk) * qj[K] + c2
    cb = cc * (ir[P] * ir[K])
    ca = cc * (cs * ir2[P]) + third
    term = np.stack([ca, cb * bx, cb * by, cb * bz], axis=1)
    assert term.dtype == np.dtype(T)
    s = _sum_rows(m, P, term, rng)
    rad = (T(0.5) * b) * Uj
    if defect != "no P_j term":
        rad = rad + (w * Pj) * S
    sat = s[:, 0] + rad
    Fj = np.stack([s[:, 1] - sat * ax, s[:, 2] - sat * ay, s[:, 3] - sat * az], axis=1)
    own = _sum_rows(n, I, np.stack([fx, fy, fz, T(0.5) * pe], axis=1), rng)
    centre = _sum_rows(n, Ie, np.concatenate([Fj, ej[:, None]], axis=1), rng)
    share_i, share_j = (T(0.5), T(0)) if defect == "pe quarters misplaced" else (T(0.25), T(0.25))
    own = own + np.concatenate([-centre[:, :3], (centre[:, 3] * share_i)[:, None]], axis=1)
    f = _sum_rows(n, np.concatenate([np.arange(n), Je]), np.concatenate([own, np.concatenate([Fj, (ej * share_j)[:, None]], axis=1)]), rng)
    assert f.dtype == np.dtype(T) and Fj.dtype == np.dtype(T)
    wv = None
    if totals:
        av = (ax, ay, az)
        three = [T(-1) * (av[c] * Fj[:, dd]) for c, dd in _AB]
        assert all(v.dtype == np.dtype(T) for v in three)
        three = [2.0 * v.astype(np.float64) for v in three] + [(2.0 if defect == "a bond twice in U" else 1.0) * ej.astype(np.float64)]
        pair_terms = [fx * dx, fy * dy, fz * dz, fx * dy, fx * dz, fy * dz, pe]
        wv = np.concatenate([_virial_tree(n, I, pos, pair_terms, e, lane3, three), [0.5 * (in_p | in3).sum()]])
    return f, wv

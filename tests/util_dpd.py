"""What tests/test_dpd.py checks the DPD pair thermostat against (nl_set_dpd, nl_dpd_forces, nl_dpd_virial; DESIGN.md section
8x): an O(N^2) float64 evaluation of the rule of include/nl_hip.h on the caller's double tables, a numpy emulation of the
kernel's arithmetic in the position type, and the velocities, tables and parameters the tests use.  No list is used, the
library's or the oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S defined here.

The inputs are the table family's of tests.consumer_util (the 2744-particle lattice, its boxes, R_MIN and R_MAX, whose bands no
pair lies in) with seeded velocities that float32 holds exactly.  Two kinds:
  * "one":    the Morse pair table of one type, one gamma and one sigma;
  * "typed3": the Morse tables of three types, whose type table leaves the pairs (0, 2) out of the list, and a gamma and a
              sigma per slot (one slot is pure friction, one has neither).
The weight table is Groot and Warren's w = 1 - r / r_max as A = w / r on (R_MIN, R_MAX) with NKD knots: a grid of its own.
"""
import functools

import numpy as np

from md_neighbor_list_amd import dpd, pair_table, rdf
from tests.consumer_util import N, NK, R_MAX, R_MIN, _tab
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, emulate_pairs, lj_pairs
from tests.util_table import _knot, _slots, _sum_rows, table_device_form, table_pairs, table_virial_emulate
from tests.virial_util import _AB

# 4 x the largest ratio of test_dpd.test_emulation_gives_c: forces and energies per particle (fp32 emulation), and the 7 totals
# (emulated in fp32 and fp64 with the kernels' own summation tree).  The measured maxima stand beside them.
EMULATED_MAX, EMULATED_MAX_W = 2.6, 0.661  # measured: 2.599 per particle (pe; forces 1.603) and 0.6606 for the totals (U, fp64)
DPD_C = 10.4
DPD_CW = 2.65

KINDS = ("one", "typed3")
NKD = 384
DT, KT, SEED, STEP = 0.01, 1.0, 12345, 7
GAMMA = 4.5


# ------------------------------------------------------------------------------------------ velocities, tables, parameters
@functools.lru_cache(maxsize=None)
def velocities(n=N, seed=23):
    """(n, 3) float64 holding float32 values: a seeded Maxwell distribution at kT = 1 plus a common drift, so that a sign
    or an order mistake in v_i - v_j shows."""
    rng = np.random.default_rng(seed)
    v = (rng.normal(size=(n, 3)) + np.array([0.25, -0.5, 0.125])).astype(np.float32).astype(np.float64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def weight_tab(nk=NKD, r_min=R_MIN, r_max=R_MAX):
    return dpd.weight(r_min, r_max, nk)


def pair_tab(kind, nk=NK):
    """(F, U, types, rc_ab) of the kind's pair table (tests.consumer_util _tab)."""
    return _tab("morse" if kind == "one" else kind, nk)


@functools.lru_cache(maxsize=None)
def params(kind):
    """(gamma, sigma) per slot: sigma = sqrt(2 gamma kT) but for the slot (1, 1) of typed3, which is pure friction; the slot
    (0, 1) has neither."""
    if kind == "one":
        g = np.array([GAMMA])
        return g, dpd.sigma_for(g, KT)
    g = np.array([GAMMA, 0.0, 3.0, 2.0, 6.0, 1.5])
    s = dpd.sigma_for(g, KT)
    s[rdf.slot(1, 1, 3)] = 0.0
    return g, s


class Model:
    """The tables and parameters of one evaluation: the pair table (F, U) on (r_min, r_max), the weight table A on
    (r_min_d, r_max_d), gamma and sigma per slot, dt, the seed and, with more than one type, the types and the type
    table's cut-offs."""

    def __init__(self, F, U, r_min, r_max, A, r_min_d, r_max_d, gamma, sigma, dt=DT, seed=SEED, types=None, rc_ab=None):
        self.F, self.U, self.r_min, self.r_max = F, U, r_min, r_max
        self.A, self.r_min_d, self.r_max_d = np.asarray(A, dtype=np.float64), r_min_d, r_max_d
        self.gamma, self.sigma = np.atleast_1d(np.asarray(gamma, dtype=np.float64)), np.atleast_1d(np.asarray(sigma, dtype=np.float64))
        self.dt, self.seed, self.types, self.rc_ab = float(dt), int(seed), types, rc_ab
        self.nt = int(round(((8 * len(self.gamma) + 1) ** 0.5 - 1) / 2))
        assert r_max == r_max_d, "the references take one pair set: both ranges end at the same r_max"
        assert rdf.nslots(self.nt) == len(self.gamma) == len(self.sigma) and (self.nt == 1 or types is not None)

    def slots(self, I, J):
        return _slots(None if self.types is None else np.asarray(self.types, dtype=np.int64), self.nt, I, J)


@functools.lru_cache(maxsize=None)
def model(kind, nk=NK, nkd=NKD, seed=SEED):
    F, U, types, rc_ab = pair_tab(kind, nk)
    g, s = params(kind)
    return Model(F, U, R_MIN, R_MAX, weight_tab(nkd), R_MIN, R_MAX, g, s, DT, seed, types, None if rc_ab is None else rc_ab(3.4))


# -------------------------------------------------------------------------------------------------------- reference
def dpd_pairs(q, v, m, step, pairs):
    """Per ordered pair that the list holds and that lies within r_max: (I, J, d, fr, pe, mf, mu) in float64 -- the pair
    table's values of tests.util_table table_pairs plus the friction -g a^2 (d . dv) and the noise sg a xi, a =
    dpd.interpolate on the weight table, xi = dpd.pair_noise, and the uncancelled magnitudes: with mA = |A_k| + |A_k+1| +
    |dA_k| r2 / D (the conditioning of s on the rounding of r2; mA >= |a|) and mdot = sum_c |d_c| (|v_ic| + |v_jc|) (the
    conditioning of dot on the rounding of dv), the friction's is g mA^2 mdot and the noise's sg mA |xi|."""
    I, J, d, fr, pe, mf, mu = table_pairs(q, m.F, m.U, m.r_min, m.r_max, pairs, m.types, m.rc_ab)
    v = np.asarray(v, dtype=np.float64)
    r2 = (d * d).sum(axis=1)
    a, inn = dpd.interpolate(m.A, m.r_min_d, m.r_max_d, r2)
    assert inn.all()
    nk = len(m.A)
    D = pair_table.spacing(m.r_min_d, m.r_max_d, nk)
    k = np.clip(((r2 - float(m.r_min_d) ** 2) / D).astype(np.int64), 0, nk - 2)
    mA = np.abs(m.A[k]) + np.abs(m.A[k + 1]) + np.abs(m.A[k + 1] - m.A[k]) * r2 / D
    sl = m.slots(I, J)
    g, sg = m.gamma[sl], (m.sigma / np.sqrt(m.dt))[sl]
    dv = v[I] - v[J]
    dot = (d * dv).sum(axis=1)
    mdot = (np.abs(d) * (np.abs(v[I]) + np.abs(v[J]))).sum(axis=1)
    xi = dpd.pair_noise(I, J, m.seed, step)
    fdpd = -(g * a * a) * dot + sg * a * xi
    below = np.isnan(a)
    return I, J, d, fr + fdpd, np.where(below, np.nan, pe), mf + g * mA * mA * mdot + sg * mA * np.abs(xi), mu


def dpd_reference(q, v, box6, mask, m, step, pairs=None):
    """(forces (want[n, 4], S[n, 4]), totals (want[8], S[7])): the layouts of tests.util_table table_reference and
    table_virial_reference; the totals summed in long double, every unordered pair once."""
    n = len(q)
    pairs = lj_pairs(q, box6, mask, float(m.r_max)) if pairs is None else pairs
    I, J, d, fr, pe, mf, mu = dpd_pairs(q, v, m, step, pairs)
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fr * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=mf * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=0.5 * pe, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n)
    assert np.finfo(np.longdouble).nmant >= 63, "dpd_reference needs an extended-precision long double"
    fl, pl, dl = fr.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    n_in = np.nan if np.isnan(fr).any() else 0.5 * len(I)  # (a pair below either table: all 8 are NaN)
    ww = np.array([float(0.5 * (fl * dl[:, a] * dl[:, b]).sum()) for a, b in _AB] + [float(0.5 * pl.sum()), n_in])
    SW = np.array([0.5 * (mf * np.abs(d[:, a] * d[:, b])).sum() for a, b in _AB] + [0.5 * mu.sum()])
    return (want, S), (ww, SW)


@functools.lru_cache(maxsize=None)
def ref(box, drift, kind, step=STEP):
    box6, mask = LJ_BOXES[box]
    return dpd_reference(_input(box, drift), velocities(), box6, mask, model(kind), step, _pairs(box, drift))


@functools.lru_cache(maxsize=None)
def moved_ref(box, kind, step=STEP):
    box6, mask = LJ_BOXES[box]
    q, pairs = _moved(box, 21)
    return dpd_reference(q, velocities(), box6, mask, model(kind), step, pairs)


def listed(m, I, J):
    """The ordered pairs (I, J) less those the type table leaves out of the list."""
    if m.rc_ab is None:
        return I, J
    keep = np.asarray(m.rc_ab)[m.types[I], m.types[J]] > 0
    return I[keep], J[keep]


# -------------------------------------------------------------------------------------------------------- emulation
DEFECTS = ("unsymmetrised key", "step + 1", "A for A A", "sigma without 1/sqrt(dt)", "friction sign", "vj - vi", "wrong slot",
           "reaction without the DPD term")


def _read(V, dV, sl, k, t, below, T):
    return np.where(below, T(np.nan), V[sl, k] + t * dV[sl, k])


def _noise_int(I, J, seed, step, symmetric=True):
    """dpd.pair_noise_int, or, unsymmetrised, the integer of the key (i << 32 | j)."""
    if symmetric:
        return dpd.pair_noise_int(I, J, seed, step)
    with np.errstate(over="ignore"):
        z = dpd.fin(dpd.pair_key(seed, step) + ((I.astype(np.uint64) << np.uint64(32)) | J.astype(np.uint64)))
    return 2 * (z >> np.uint64(40)).astype(np.int64) + 1 - (1 << 24)


def dpd_emulate_pairs(q, v, box6, mask, m, step, T, pairs, defect=None):
    """lj_image (tests.util emulate_pairs) and DpdByPair::entry and ::pair (csrc/nl_dpd.inc) in the position type T over the
    ordered pairs (I, J): one rounding per operation, no FMA.  Returns (dx, dy, dz, fx, fy, fz, pe, in) in T.  defect: one of
    DEFECTS, the deliberate mistakes of test_wrong_results_are_rejected."""
    assert defect is None or defect in DEFECTS
    T = np.dtype(T).type
    I, J = pairs[0], pairs[1]
    dx, dy, dz = emulate_pairs(q, box6, mask, 1.0, 1.0, 1.0, T, pairs)[:3]
    r2 = dx * dx + dy * dy + dz * dz
    Ft, dFt, Ut, dUt, x0, xc, iD = table_device_form(m.F, m.U, m.r_min, m.r_max, T)
    nslots, nk = Ft.shape
    nt = int(round(((8 * nslots + 1) ** 0.5 - 1) / 2))
    sl = _slots(None if m.types is None else np.asarray(m.types, dtype=np.int64), nt, I, J)
    in_p, below, k, t = _knot(r2, x0, xc, iD, nk, T)
    frp = np.where(in_p, _read(Ft, dFt, sl, k, t, below, T), T(0))
    pep = np.where(in_p, _read(Ut, dUt, sl, k, t, below, T), T(0))
    At, dAt, _, _, x0d, xcd, iDd = table_device_form(m.A, np.zeros_like(m.A), m.r_min_d, m.r_max_d, T)
    in_d, below_d, k, t = _knot(r2, x0d, xcd, iDd, At.shape[1], T)
    A = _read(At, dAt, np.zeros(len(I), dtype=np.int64), k, t, below_d, T)
    sd = m.slots(I, J)
    if defect == "wrong slot":
        sd = (sd + 1) % len(m.gamma)
    g = m.gamma.astype(T)[sd]
    sg = (m.sigma if defect == "sigma without 1/sqrt(dt)" else m.sigma / np.sqrt(m.dt)).astype(T)[sd]
    vt = np.asarray(v)[:, :3].astype(T)
    dv = vt[J] - vt[I] if defect == "vj - vi" else vt[I] - vt[J]
    dot = (dx * dv[:, 0] + dy * dv[:, 1]) + dz * dv[:, 2]
    mi = _noise_int(I, J, m.seed, step + 1 if defect == "step + 1" else step, defect != "unsymmetrised key")
    xi = mi.astype(T) * T(dpd.XI_SCALE)
    fd = (g * A) * dot if defect == "A for A A" else (g * (A * A)) * dot
    if defect != "friction sign":
        fd = -fd
    fn = (sg * A) * xi
    fdpd = np.where(in_d, fd + fn, T(0))
    if defect == "reaction without the DPD term":  # a half list stores (i, j), i < j: what j receives is the ordered pair (j, i)
        fdpd = np.where(I < J, fdpd, T(0))
    fr = frp + fdpd
    pe = np.where(in_d & below_d, T(np.nan), pep)
    out = (dx, dy, dz, fr * dx, fr * dy, fr * dz, pe, in_p | in_d)
    assert all(o.dtype == np.dtype(T) for o in out[:7])
    return out


def dpd_emulate(q, v, box6, mask, m, step, T, rng, pairs, defect=None):
    """The row body of k_dpd_forces over dpd_emulate_pairs' values, f = {fx, fy, fz, pe / 2} summed per particle in T, every
    particle's terms in a random order (tests.util_table _sum_rows).  Returns f[n, 4] in T."""
    T = np.dtype(T).type
    _, _, _, fx, fy, fz, pe, _ = dpd_emulate_pairs(q, v, box6, mask, m, step, T, pairs, defect)
    term = np.stack([fx, fy, fz, T(0.5) * pe], axis=1)
    assert term.dtype == np.dtype(T)
    return _sum_rows(len(q), pairs[0], term, rng)


def dpd_virial_emulate(n, I, vals, rng):
    """k_dpd_virial and k_virial_reduce over dpd_emulate_pairs' values of a full list, with the kernels' own summation tree
    (tests.util_table table_virial_emulate: the kernels are the table kernels with another pair function)."""
    return table_virial_emulate(n, I, vals, rng)

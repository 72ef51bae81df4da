"""What tests/test_coulomb.py checks the charge consumer against (nl_set_coulomb_table, nl_coul_forces, nl_coul_virial;
DESIGN.md section 8u): an O(N^2) float64 evaluation of the rule of include/nl_hip.h on the caller's double tables, a numpy
emulation of the kernel's arithmetic in the position type, the charge sets and the tables the tests use.  No list is used, the
library's or the oracle's; the bound is check_lj's / check_virial's, |got - want| <= c u S, with the S defined here.

The inputs are the table family's of tests.consumer_util (the 2744-particle lattice, its boxes, R_MIN and R_MAX, whose bands no
pair lies in).  Two kinds:
  * "salt":   the Morse pair table of one type, charges +-1 by lattice parity (rock salt);
  * "typed3": the Morse tables of three types, whose type table leaves the pairs (0, 2) out of the list -- they have no charge
              term either --, and seeded random charges with |q| in [0.5, 1] and an exact zero sum.
The charge table is the real-space Ewald term, prefactor 4, on (R_MIN, R_MAX) with NKC knots: a grid of its own.
"""
import functools

import numpy as np

from md_neighbor_list_amd import coulomb, pair_table
from tests.consumer_util import N, NK, R_MAX, R_MIN, _tab
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, emulate_pairs, lj_pairs
from tests.util_table import _knot, _slots, _sum_rows, table_device_form, table_pairs, table_virial_emulate
from tests.virial_util import _AB

# 4 x the largest ratio of test_coulomb.test_emulation_gives_c: forces and energies per particle (fp32 emulation), and the 7
# totals (emulated in fp32 and fp64 with the kernels' own summation tree).  The measured maxima stand beside them.
EMULATED_MAX, EMULATED_MAX_W = 1.55, 0.432  # measured: 1.548 per particle (pe; forces 1.08) and 0.4317 for the totals (U, fp64)
COUL_C = 6.2
COUL_CW = 1.73

KINDS = ("salt", "typed3")
NKC = 512
ALPHA, PREFACTOR = 0.4, 4.0
Q_MIN = 0.5  # the smallest |q| of any charge set
# what the emulation that fixes COUL_C and COUL_CW runs over
EMULATED = [("open", False, "salt"), ("xyz", False, "salt"), ("xyz", True, "typed3"), ("tilt", False, "typed3"), ("tilt", True, "salt"),
            ("xy", True, "typed3"), ("hex", True, "salt"), ("hex", False, "typed3"), ("xy", False, "salt")]


# ---------------------------------------------------------------------------------------------------- charges, tables
@functools.lru_cache(maxsize=None)
def charges(kind):
    """(n,) float64 holding float32 values.  salt: +-1 by the parity of the lattice site; else 1372 magnitudes in
    [0.5, 1] given once to a positive and once to a negative particle, in a seeded random order: the sum is exactly 0."""
    if kind == "salt":
        g = np.stack(np.meshgrid(*(np.arange(LJ_M),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        q = np.where(g.sum(axis=1) % 2 == 0, 1.0, -1.0)
    else:
        rng = np.random.default_rng(17)
        m = rng.uniform(Q_MIN, 1.0, size=N // 2).astype(np.float32).astype(np.float64)
        q = np.empty(N)
        perm = rng.permutation(N)
        q[perm[:N // 2]], q[perm[N // 2:]] = m, -m
    assert q.sum() == 0.0 and np.abs(q).min() >= Q_MIN and np.array_equal(q, q.astype(np.float32))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def coul_tab(nk=NKC, r_min=R_MIN, r_max=R_MAX):
    """(K, C) of the charge table."""
    return coulomb.ewald_real(ALPHA, r_min, r_max, nk, prefactor=PREFACTOR)


def pair_tab(kind, nk=NK):
    """(F, U, types, rc_ab) of the kind's pair table (tests.consumer_util _tab)."""
    return _tab("morse" if kind == "salt" else kind, nk)


class Model:
    """The tables and charges of one evaluation: the pair table (F, U) on (r_min, r_max), the charge table (K, C) on
    (r_min_c, r_max_c), the charges and, for a typed pair table, the types and the type table's cut-offs."""

    def __init__(self, F, U, r_min, r_max, K, C, r_min_c, r_max_c, q, types=None, rc_ab=None):
        self.F, self.U, self.r_min, self.r_max = F, U, r_min, r_max
        self.K, self.C, self.r_min_c, self.r_max_c = K, C, r_min_c, r_max_c
        self.q, self.types, self.rc_ab = np.asarray(q, dtype=np.float64), types, rc_ab
        assert r_max == r_max_c, "the references take one pair set: both ranges end at the same r_max"


@functools.lru_cache(maxsize=None)
def model(kind, nk=NK, nkc=NKC):
    F, U, types, rc_ab = pair_tab(kind, nk)
    K, C = coul_tab(nkc)
    return Model(F, U, R_MIN, R_MAX, K, C, R_MIN, R_MAX, charges(kind), types, None if rc_ab is None else rc_ab(3.4))


# -------------------------------------------------------------------------------------------------------- reference
def coul_pairs(q, m, pairs):
    """Per ordered pair that the list holds and that lies within r_max: (I, J, d, fr, pe, mf, mu) in float64 -- the pair
    table's values of tests.util_table table_pairs plus q_i q_j times coulomb.interpolate on the charge table, and the
    uncancelled magnitudes of both: for either table |V_k| + |V_k+1| + |dV_k| r2 / D, the third term the conditioning of
    s = (r2 - x0) / D on the rounding of r2, the charge table's times |q_i q_j|."""
    I, J, d, fr, pe, mf, mu = table_pairs(q, m.F, m.U, m.r_min, m.r_max, pairs, m.types, m.rc_ab)
    r2 = (d * d).sum(axis=1)
    qq = m.q[I] * m.q[J]
    kc, cc, inn = coulomb.interpolate(m.K, m.C, m.r_min_c, m.r_max_c, r2)
    assert inn.all()
    nk = len(m.K)
    D = pair_table.spacing(m.r_min_c, m.r_max_c, nk)
    k = np.clip(((r2 - float(m.r_min_c) ** 2) / D).astype(np.int64), 0, nk - 2)
    mag = [np.abs(t[k]) + np.abs(t[k + 1]) + np.abs(t[k + 1] - t[k]) * r2 / D for t in (m.K, m.C)]
    return I, J, d, fr + qq * kc, pe + qq * cc, mf + np.abs(qq) * mag[0], mu + np.abs(qq) * mag[1]


def coul_reference(q, box6, mask, m, pairs=None):
    """(forces (want[n, 4], S[n, 4]), totals (want[8], S[7])): the layouts of tests.util_table table_reference and
    table_virial_reference; the totals summed in long double, every unordered pair once."""
    n = len(q)
    pairs = lj_pairs(q, box6, mask, float(m.r_max)) if pairs is None else pairs
    I, J, d, fr, pe, mf, mu = coul_pairs(q, m, pairs)
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fr * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=mf * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=0.5 * pe, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n)
    assert np.finfo(np.longdouble).nmant >= 63, "coul_reference needs an extended-precision long double"
    fl, pl, dl = fr.astype(np.longdouble), pe.astype(np.longdouble), d.astype(np.longdouble)
    n_in = np.nan if np.isnan(fr).any() else 0.5 * len(I)  # (a pair below either table: all 8 are NaN)
    ww = np.array([float(0.5 * (fl * dl[:, a] * dl[:, b]).sum()) for a, b in _AB] + [float(0.5 * pl.sum()), n_in])
    SW = np.array([0.5 * (mf * np.abs(d[:, a] * d[:, b])).sum() for a, b in _AB] + [0.5 * mu.sum()])
    return (want, S), (ww, SW)


@functools.lru_cache(maxsize=None)
def ref(box, drift, kind):
    box6, mask = LJ_BOXES[box]
    return coul_reference(_input(box, drift), box6, mask, model(kind), _pairs(box, drift))


@functools.lru_cache(maxsize=None)
def moved_ref(box, kind, seed=21):
    box6, mask = LJ_BOXES[box]
    q, pairs = _moved(box, seed)
    return coul_reference(q, box6, mask, model(kind), pairs)


def listed(m, I, J):
    """The ordered pairs (I, J) less those the type table leaves out of the list."""
    if m.rc_ab is None:
        return I, J
    keep = np.asarray(m.rc_ab)[m.types[I], m.types[J]] > 0
    return I[keep], J[keep]


def weakest(m):
    """(force component, energy) the weakest single charged pair at r_max_c gives a particle through the charge term alone,
    for charges no smaller than Q_MIN: |q_i q_j| K(r_max) r_max / sqrt(3) (a separation has a component of at least
    r / sqrt(3)) and |q_i q_j| |C(r_max)| / 2."""
    qq = np.abs(m.q).min() ** 2
    return qq * abs(m.K[-1]) * m.r_max_c / np.sqrt(3.0), 0.5 * qq * abs(m.C[-1])


# -------------------------------------------------------------------------------------------------------- emulation
DEFECTS = ("qj for qq", "the row's charge for the partner's", "C and K swapped", "no charge term in pe", "reaction without qq")


def _read(V, dV, sl, k, t, below, T):
    return np.where(below, T(np.nan), V[sl, k] + t * dV[sl, k])


def coul_emulate_pairs(q, box6, mask, m, T, pairs, defect=None):
    """lj_image (tests.util emulate_pairs) and CoulByPair::pair (csrc/nl_coulomb.inc) in the position type T over the ordered
    pairs (I, J): one rounding per operation, no FMA.  Returns (dx, dy, dz, fx, fy, fz, pe, in) in T.  defect: one of DEFECTS,
    the deliberate mistakes of test_wrong_results_are_rejected."""
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
    Kt, dKt, Ct, dCt, x0c, xcc, iDc = table_device_form(m.K, m.C, m.r_min_c, m.r_max_c, T)
    if defect == "C and K swapped":
        Kt, dKt, Ct, dCt = Ct, dCt, Kt, dKt
    in_c, below, k, t = _knot(r2, x0c, xcc, iDc, Kt.shape[1], T)
    qt = m.q.astype(T)
    qi, qj = qt[I], qt[J]
    qq = qi * qj
    if defect == "qj for qq":
        qq = qj
    elif defect == "the row's charge for the partner's":
        qq = qi * qi
    elif defect == "reaction without qq":  # a half list stores (i, j), i < j: what j receives is the ordered pair (j, i)
        qq = np.where(I < J, qq, T(1))
    zero = np.zeros(len(I), dtype=np.int64)
    fc = np.where(in_c, qq * _read(Kt, dKt, zero, k, t, below, T), T(0))
    ec = np.where(in_c, qq * _read(Ct, dCt, zero, k, t, below, T), T(0))
    fr = frp + fc
    pe = pep if defect == "no charge term in pe" else pep + ec
    out = (dx, dy, dz, fr * dx, fr * dy, fr * dz, pe, in_p | in_c)
    assert all(v.dtype == np.dtype(T) for v in out[:7])
    return out


def coul_emulate(q, box6, mask, m, T, rng, pairs, defect=None):
    """The row body of k_coul_forces over coul_emulate_pairs' values, f = {fx, fy, fz, pe / 2} summed per particle in T, every
    particle's terms in a random order (tests.util_table _sum_rows).  Returns f[n, 4] in T."""
    T = np.dtype(T).type
    _, _, _, fx, fy, fz, pe, _ = coul_emulate_pairs(q, box6, mask, m, T, pairs, defect)
    term = np.stack([fx, fy, fz, T(0.5) * pe], axis=1)
    assert term.dtype == np.dtype(T)
    return _sum_rows(len(q), pairs[0], term, rng)


def coul_virial_emulate(n, I, vals, rng):
    """k_coul_virial and k_virial_reduce over coul_emulate_pairs' values of a full list, with the kernels' own summation tree
    (tests.util_table table_virial_emulate: the kernels are the table kernels with another pair function)."""
    return table_virial_emulate(n, I, vals, rng)

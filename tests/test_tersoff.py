"""Tersoff bond-order potentials (nl_set_tersoff, nl_tersoff_forces, nl_tersoff_virial and their enqueue variants) against a
float64 evaluation of the rule, with an error bound per particle and per component.

Contract tested (include/nl_hip.h, nl_set_tersoff):
  * |got - want| <= TERSOFF_C u S for every particle and each of fx, fy, fz, pe on its own, and <= TERSOFF_CW u S for each of the
    7 sums of the totals, n_in exact.  want: tests.util_tersoff tf_reference (md_neighbor_list_amd.tersoff bond_energy and
    pair_table.interpolate on the caller's double tables over an O(N^2) pair sweep, no list).  S: the uncancelled sums of a
    first-order error propagation through the rule (tf_reference's docstring), with the three terms of every table read, the
    conditioning of b and b' on zeta, and |h| + |cs| where the error of h - cs stands;
  * NaN rules (more than 64 partners in range, a partner below the radial tables, a lone one too), LDS against global,
    reproducible totals, the enqueue variants, state and arguments.

The constants are not fitted to the kernel.  Each is 4 x the largest ratio that a numpy emulation of the stated rule in the
position type reaches against the float64 reference (tests.util_tersoff tf_emulate: one rounding per operation, no FMA, random
summation orders, knots and scalars rounded as the setter rounds them, each pow numpy's perturbed by up to POW_ULP = 2 ulp; the
totals with the kernels' summation tree) over the inputs of EMULATED, in float32 and in float64; test_emulation_gives_c
recomputes them.  Sharpness is shown by the defects of test_wrong_results_are_rejected.

The inputs are those of tests/test_pair_table.py and tests/test_sw.py: the 14^3 jittered lattice, n = 2744, on the boxes of
LJ_BOXES, in the box and drifted, and _moved: at most 49 partners within 2.5.  The test potential is in reduced units with f_C
ramping from 1.0 to 1.9, through the first two shells.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import pair_table, tersoff
from tests import consumer_contract as contract
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _bonds, _handle, _pair_tab, _tab, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_unit
from tests.util_table import _knot, _lin, morse, table_device_form
from tests.util_tersoff import (CUT_D, CUT_R, DEFECTS, POW_ULP, TERSOFF_C, TERSOFF_CW, TfTables, tf_emulate, tf_energy, tf_functions,
                                tf_parameters, tf_reference, tf_repulsive)
from tests.virial_util import check_virial, virial_ratio

KINDS = ("one", "typed3")
R_22 = 2.2  # the second range
EMULATED = [("open", False, "one"), ("xyz", False, "one"), ("tilt", True, "one"), ("xyz", True, "typed3"), ("tilt", False, "typed3"),
            ("open", False, "typed3")]
EMULATED_MAX, EMULATED_MAX_W = 2.82, 0.513  # the largest ratios of test_emulation_gives_c: per particle, and of the totals


# ------------------------------------------------------------------------------------------------ inputs, references
def _radial(nt, lam3, r_min_3, r_max_3, nk, R=CUT_R, D=CUT_D):
    us, dus, qs, dqs, ps, dps = tf_functions(nt, lam3=lam3, R=R, D=D)
    pick = (lambda v: v[0][0]) if nt == 1 else (lambda v: v)
    u, Uu = tersoff.sample(pick(us), pick(dus), r_min_3, r_max_3, nk)
    q, Qq = tersoff.sample(pick(qs), pick(dqs), r_min_3, r_max_3, nk)
    p, Pp = (None, None) if ps is None else tersoff.sample(pick(ps), pick(dps), r_min_3, r_max_3, nk)
    return u, Uu, q, Qq, p, Pp


@functools.lru_cache(maxsize=None)
def _tabs(kind, nk=NK, r_max_3=R_MAX, r_max_pair=R_MAX, r_min_pair=R_MIN, r_min_3=R_MIN, pair=True, bond=True, beta=True):
    """(TfTables, types, rc_ab(rc_list)) of a potential.  "one": one type, the Morse pair table, p = NULL.  "typed3": the 3-type
    mixture of test_pair_table's typed3, whose pair (0, 2) the type table leaves out of the list, lambda_3 != 0, nine slots not
    symmetric in (centre, end), 27 angular sets not symmetric in the ends.  pair=False: a zero pair table; bond=False: u = U = 0;
    beta=False: beta = 0."""
    nt = 1 if kind == "one" else 3
    F, U, types, rc_ab = _tab("morse" if nt == 1 else "typed3", nk)
    if (r_min_pair, r_max_pair) != (R_MIN, R_MAX):
        F, U = _pair_tab(nt, r_min_pair, r_max_pair, nk)
    u, Uu, q, Qq, p, Pp = _radial(nt, nt > 1, r_min_3, r_max_3, nk)
    par = list(tf_parameters(nt))
    if not bond:
        u, Uu = np.zeros_like(u), np.zeros_like(Uu)
    if not pair:
        F, U = np.zeros_like(F), np.zeros_like(U)
    if not beta:
        par[4] = np.zeros_like(par[4])
    return TfTables(F, U, r_min_pair, r_max_pair, u, Uu, q, Qq, p, Pp, r_min_3, r_max_3, *par), types, rc_ab


def _refs(q, box, kind, pairs, exclusions=None, **kw):
    box6, mask = LJ_BOXES[box]
    tab, types, rc_ab = _tabs(kind, **kw)
    return tf_reference(q, box6, mask, tab, pairs, types=types, rc_ab=None if rc_ab is None else rc_ab(3.4), exclusions=exclusions)


@functools.lru_cache(maxsize=None)
def _ref(box, drift, kind):
    return _refs(_input(box, drift), box, kind, _pairs(box, drift))


@functools.lru_cache(maxsize=None)
def _moved_ref(box, kind, seed=21):
    q, pairs = _moved(box, seed)
    return _refs(q, box, kind, pairs)


# ------------------------------------------------------------------------------------------------- CPU: the checker
def test_header_states_the_constants():
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    assert int(re.search(r"#define NL_TERSOFF_MAX_TYPES\s+(\d+)", text).group(1)) == 4 == tersoff.MAX_TYPES
    assert int(re.search(r"#define NL_TERSOFF_MAX_NEAR\s+(\d+)", text).group(1)) == 64 == tersoff.MAX_NEAR
    for name in ("nl_set_tersoff", "nl_get_tersoff", "nl_tersoff_forces", "nl_tersoff_forces_enqueue", "nl_tersoff_virial",
                 "nl_tersoff_virial_enqueue"):
        assert re.search(r"\bint %s\(" % name, text), name
    assert "3.8e7" in text and "2 ulp" in text  # the reason for the rearranged g, and the accuracy assumed of pow


def test_inputs():
    """On the inputs b spreads over roughly 0.3 to 0.95 and g by far more than a factor of 2, in both sets; no centre has more
    than 49 partners in range; the typed set is not symmetric where the rule is not."""
    for kind in KINDS:
        ref = _ref("xyz", False, kind)
        tab = _tabs(kind)[0]
        Ie, Je, ej = ref["ends"]
        live = ej != 0  # (beyond f_C a bond carries nothing)
        b, g = ref["b"][live], ref["g"]
        print(kind, "b", np.percentile(b, [0, 1, 50, 99, 100]).round(3), "g", np.percentile(g, [0, 1, 50, 99, 100]).round(3), "bonds", live.sum())
        assert b.min() < 0.4 and b.max() > 0.85 and np.percentile(b, 99) / np.percentile(b, 1) > 1.9
        assert np.percentile(g, 95) / np.percentile(g, 5) > 2.0
        assert ref["near"].max() <= 49 < tersoff.MAX_NEAR and live.sum() > 8 * N
        assert np.isfinite(ref["want"]).all() and np.abs(ref["bond"][:, :3]).max() > 1.0
        assert (tab.p is None) == (kind == "one")
    tab, types, rc_ab = _tabs("typed3")
    assert tab.u.shape == (9, NK) and not np.allclose(tab.u[1], tab.u[3]) and not np.allclose(tab.q[1], tab.q[3]) and rc_ab(3.4)[0, 2] == 0
    assert all(not np.allclose(a, a.transpose(0, 2, 1)) for a in tab.ang) and not np.allclose(tab.beta, tab.beta.T)
    assert len(np.unique(tab.ang[0])) >= 14


def test_rearranged_g_is_the_lammps_form():
    """gamma + gc x2 / den against gamma (1 + c^2/d^2 - c^2 / (d^2 + (h - cs)^2)) in float64, and g' against its central
    difference; with silicon's parameters the LAMMPS form loses 7 digits to the subtraction, so the comparison is relative to
    gamma c^2/d^2."""
    cs = np.linspace(-1.0, 1.0, 2001)
    for gamma, c, d, h in ((1.0, 1.0, 0.15, 0.0), (0.02, 1.2, 0.4, -0.3), (1.0, 100390.0, 16.217, -0.59825)):
        par = [v[0, 0, 0] for v in tersoff.angular(gamma, c, d, h)]
        g, gp = tersoff.g_of(cs, *par)
        lammps = gamma * (1.0 + c * c / (d * d) - c * c / (d * d + (h - cs) ** 2))
        assert np.abs(g - lammps).max() <= 8 * np.finfo(np.float64).eps * gamma * (1.0 + c * c / (d * d))
        e = 1e-6
        fd = (tersoff.g_of(cs + e, *par)[0] - tersoff.g_of(cs - e, *par)[0]) / (2 * e)
        assert np.abs(gp - fd).max() <= 1e-6 * np.abs(gp).max()
    b, bp = tersoff.b_of(np.array([-1.0, 0.0, 0.5, 2.0, np.nan]), 1.1, 2.5)
    assert b[0] == b[1] == 1 and bp[0] == bp[1] == 0 and np.isnan(b[4]) and np.isnan(bp[4]) and 0 < b[3] < b[2] < 1
    e = 1e-6
    assert abs((tersoff.b_of(2.0 + e, 1.1, 2.5)[0] - tersoff.b_of(2.0 - e, 1.1, 2.5)[0]) / (2 * e) - bp[3]) < 1e-8


def test_sampled_tables_converge():
    """The radial tables against the functions they sample, on a dense grid: the largest error falls 4 x per doubling of the knots.
    The second derivative of the LAMMPS f_C jumps at both ends of its ramp, so F = -f'/r has a kink there: in the two segments that
    hold the kinks the error of U and Q falls about 2 x, depending on where in its segment a kink lies (asserted: it falls); they are
    left out of the 4 x."""
    us, dus, qs, dqs, ps, dps = tf_functions(3)
    x = np.linspace(0.92 ** 2, R_MAX ** 2, 100001)[:-1]
    r = np.sqrt(x)
    worst, at_kinks = [], []
    for nk in (512, 1024, 2048, 4096):
        w, wk = [], []
        D = pair_table.spacing(R_MIN, R_MAX, nk)
        smooth = (np.abs(x - (CUT_R - CUT_D) ** 2) > D) & (np.abs(x - (CUT_R + CUT_D) ** 2) > D)
        for f, df in ((us, dus), (qs, dqs), (ps, dps)):
            v, V = tersoff.sample(f, df, R_MIN, R_MAX, nk)
            for s, (a, b) in enumerate([(a, b) for a in range(3) for b in range(3)]):
                Vv, vv, inn = pair_table.interpolate(V[s], v[s], R_MIN, R_MAX, x)
                assert inn.all()
                w += [np.abs(vv - f[a][b](r)).max(), np.abs(Vv + df[a][b](r) / r)[smooth].max()]
                wk.append(np.abs(Vv + df[a][b](r) / r).max())
        worst.append(w), at_kinks.append(wk)
    ratios, rk = np.array(worst[:-1]) / np.array(worst[1:]), np.array(at_kinks[:-1]) / np.array(at_kinks[1:])
    print("ratios", ratios.min().round(2), ratios.max().round(2), "with the kinks", rk.min().round(2), rk.max().round(2))
    assert np.all((ratios > 3.0) & (ratios < 5.0)) and np.all((rk > 1.2) & (rk < 5.0))
    fc, dfc = tersoff.cutoff(2.85, 0.15)
    assert fc(2.7) == 1 and fc(3.0) == 0 and fc(3.1) == 0 and dfc(3.0) == 0 and dfc(2.69) == 0 and abs(fc(2.85) - 0.5) < 1e-15
    with pytest.raises(ValueError):
        tersoff.bond_order(1.0, 0.0)
    with pytest.raises(ValueError):
        tersoff.angular(1.0, 1.0, 0.0, 0.0)


def _cluster():
    """A 5^3 two-type cluster in a tilted periodic box, its analytic functions (f_C from 0.9 to 1.7, inside the tables' 1.8) and
    the tables of them at nk knots."""
    rng = np.random.default_rng(3)
    m, a0 = 5, 1.125
    box6, mask = (m * a0, m * a0, m * a0, a0, -a0, 2 * a0), 7
    grid = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (grid + 0.5) * a0 + rng.uniform(-0.1, 0.1, size=grid.shape)
    types = rng.integers(0, 2, size=len(q))
    R, D = 1.3, 0.4
    us, dus, qs, dqs, ps, dps = tf_functions(2, R=R, D=D)
    phi, dphi = tf_repulsive(2, R, D)
    par = tf_parameters(2)

    def tables(nk, r_min=0.5, r_max=1.8):
        rows = [pair_table.sample(phi[a][b], dphi[a][b], r_min, r_max, nk) for a in range(2) for b in range(a, 2)]
        F, U = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        rad = [tersoff.sample(f, df, r_min, r_max, nk) for f, df in ((us, dus), (qs, dqs), (ps, dps))]
        return TfTables(F, U, r_min, r_max, rad[0][0], rad[0][1], rad[1][0], rad[1][1], rad[2][0], rad[2][1], r_min, r_max, *par)

    return q, types, box6, mask, (phi, us, qs, ps), par, tables


def test_reference_is_the_gradient_of_its_energy():
    """tf_reference's forces at 4096 knots against the central difference of the ANALYTIC float64 energy (tf_energy: the textbook
    form, the LAMMPS g, independent of bond_energy) on a two-type cluster, tilted and periodic.  The tolerance is the interpolation
    error the forces carry, measured through the rule itself: the error falls 4 x per doubling of the knots (asserted), so the
    difference between the forces at 4096 and at 8192 knots is 3/4 of the error at 4096.  Momentum: sum F = 0 within rounding."""
    q, types, box6, mask, fns, par, tables = _cluster()
    h = 1e-5
    pairs = lj_pairs(q, box6, mask, 1.8)
    refs = {nk: tf_reference(q, box6, mask, tables(nk), pairs, types=types) for nk in (2048, 4096, 8192)}
    f2, f4, f8 = (refs[nk]["want"][:, :3] for nk in (2048, 4096, 8192))
    d48, d24 = np.abs(f4 - f8).max(axis=1), np.abs(f2 - f4).max(axis=1)
    print("carried interpolation error, largest:", d48.max() * 4 / 3, "falls by", np.median(d24 / d48))
    assert 3.0 < np.median(d24 / d48) < 5.0 and d48.max() < 1e-4 * np.abs(f4).max()
    carried = (4.0 / 3.0) * np.maximum(d48, np.median(d48))
    ref = refs[4096]
    assert np.abs(np.sqrt(ref["entries"][3]) - 1.8).min() > 10 * h and ref["near"].max() > 8
    for i in range(4):
        for c in range(3):
            en = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                en.append(tf_energy(p, fns, par, 1.8, lj_pairs(p, box6, mask, 1.8), types))
            fd = -(en[0] - en[1]) / (2 * h)
            tol = 1.5 * carried[i] + 1e-8 * ref["S"][i, c]
            assert abs(fd - ref["want"][i, c]) <= tol, (i, c, fd, ref["want"][i, c], tol)
    assert np.abs(ref["want"][:, :3].sum(axis=0)).max() <= 1e-12 * ref["S"][:, :3].sum()  # Newton's third law
    assert abs(ref["ww"][6] - ref["want"][:, 3].sum()) <= 1e-12 * ref["SW"][6]
    assert abs(ref["ww"][6] - tf_energy(q, fns, par, 1.8, pairs, types)) < 1e-4


def test_a_silicon_crystal():
    """A perfect diamond crystal of 4 x 4 x 4 cells, 512 atoms, a = 5.432, with silicon(): every atom has four partners at
    r0 = a sqrt(3) / 4 inside f_C = 1 and every angle is the tetrahedral one, so zeta = 3 g(-1/3) and
    E / N = 2 [f_R(r0) + b(zeta) f_A(r0)] -- derived here from the parameters -- within the interpolation error.  (It evaluates
    to -4.6296; the published cohesive energy of the Si(C) set is 4.63 eV, recorded, not asserted.)"""
    si = tersoff.silicon()
    a0 = 5.432
    r0 = a0 * np.sqrt(3.0) / 4.0
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]) / 4.0
    cells = np.stack(np.meshgrid(*(np.arange(4),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) + 0.125) * a0
    n = len(q)
    r_min, r_max, nk = 1.5, si["R"] + si["D"], 2048
    fr, dfr = tersoff.repulsive(si["A"], si["lam1"], si["R"], si["D"])
    fa, dfa = tersoff.attractive(si["B"], si["lam2"], si["R"], si["D"])
    (fq, dfq), _ = tersoff.zeta_radial(si["lam3"], si["R"], si["D"])
    F, U = pair_table.sample(fr, dfr, r_min, r_max, nk)
    u, Uu = tersoff.sample(fa, dfa, r_min, r_max, nk)
    qq, Qq = tersoff.sample(fq, dfq, r_min, r_max, nk)
    par = tersoff.angular(si["gamma"], si["c"], si["d"], si["h"]) + tersoff.bond_order(si["beta"], si["n"])
    tab = TfTables(F, U, r_min, r_max, u, Uu, qq, Qq, None, None, r_min, r_max, *par)
    box6 = (4 * a0,) * 3 + (0.0, 0.0, 0.0)
    ref = tf_reference(q, box6, 7, tab, lj_pairs(q, box6, 7, r_max))
    assert n == 512 and np.all(ref["near"] == 4) and ref["ordered"] == 12 * n
    g = si["gamma"] * (1.0 + si["c"] ** 2 / si["d"] ** 2 - si["c"] ** 2 / (si["d"] ** 2 + (si["h"] + 1.0 / 3.0) ** 2))
    b = (1.0 + (si["beta"] * 3.0 * g) ** si["n"]) ** (-1.0 / (2.0 * si["n"]))
    closed = 2.0 * (si["A"] * np.exp(-si["lam1"] * r0) - b * si["B"] * np.exp(-si["lam2"] * r0))
    x = np.linspace(2.0 ** 2, r_max ** 2, 200001)[:-1]
    err_r = np.abs(pair_table.interpolate(F, U, r_min, r_max, x)[1] - fr(np.sqrt(x))).max()
    err_a = np.abs(pair_table.interpolate(Uu, u, r_min, r_max, x)[1] - fa(np.sqrt(x))).max()
    print("E/N", ref["ww"][6] / n, "closed form", closed, "b", b, "interpolation errors", err_r, err_a)
    assert np.allclose(ref["b"], b, rtol=1e-9, atol=0) and r0 < si["R"] - si["D"]
    assert abs(ref["ww"][6] / n - closed) <= 2.0 * (err_r + err_a) + 1e-9 and err_r + err_a < 1e-4
    assert abs(closed + 4.62960) < 1e-5
    assert np.abs(ref["want"][:, :3]).max() < 1e-9  # (every atom is a centre of symmetry of its shell)


def test_emulation_gives_c():
    """TERSOFF_C and TERSOFF_CW = 4 x the largest |emulated - want| / (u S) of the numpy emulation (never the kernel) against the
    float64 reference."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    for box, drift, kind in EMULATED:
        box6, mask = LJ_BOXES[box]
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        q = _input(box, drift)
        rng = np.random.default_rng(300)
        for T in DTYPES:  # (every constant covers both position types: in fp64 u S is only a few ulp of a result)
            f, w = tf_emulate(q, box6, mask, tab, T, rng, ref["entries"], types=types)
            r = lj_ratio(f, ref["want"], ref["S"], T).max(axis=0)
            assert w[7] == ref["ww"][7]
            rw = virial_ratio(w, ref["ww"], ref["SW"], T)
            print(box, drift, kind, np.dtype(T).name, r.round(3), rw.round(3))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, rw)
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX and TERSOFF_C == 4 * EMULATED_MAX
    assert worst_w.max() <= EMULATED_MAX_W and TERSOFF_CW == 4 * EMULATED_MAX_W


def test_wrong_results_are_rejected():
    """The checks under the fp32 bound (the totals under the fp64 bound) pass the float64 emulation of the rule and refuse each of
    DEFECTS: a dropped partner in S_j (the median of the terms that count), g_kj where g_jk belongs, the slot (t_j, t_i) for
    (t_i, t_j), the w_k term left out (the force from the neighbours' bonds), the P_j term left out (lambda_3 != 0), b' with the
    wrong sign, a bond counted twice in U (the totals alone), the quarters of pe misplaced (the per-particle energies alone)."""
    box, drift = "xyz", False
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    for kind in KINDS:
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        rng = np.random.default_rng(5)
        f, w = tf_emulate(q, box6, mask, tab, np.float64, rng, ref["entries"], types=types)
        check_lj(f, ref["want"], ref["S"], np.float32, c=TERSOFF_C)
        check_virial(w, ref["ww"], ref["SW"], np.float64, c=TERSOFF_CW)
        if kind == "one":
            continue  # (the typed defects need three types and lambda_3; the others are refused there as well)
        for defect in DEFECTS:
            f, w = tf_emulate(q, box6, mask, tab, np.float64, rng, ref["entries"], types=types, defect=defect, ulp=0)
            if defect == "a bond twice in U":
                check_lj(f, ref["want"], ref["S"], np.float32, c=TERSOFF_C)
            else:
                with pytest.raises(AssertionError):
                    check_lj(f, ref["want"], ref["S"], np.float32, c=TERSOFF_C)
            if defect != "pe quarters misplaced":  # (the totals take U from e_j itself)
                with pytest.raises(AssertionError):
                    check_virial(w, ref["ww"], ref["SW"], np.float64, c=TERSOFF_CW, count=False)
            print(kind, defect, "refused")


# ---- the 64-partner edge: test_sw's input, a centre of type 1 with donors of type 0 on interstitial sites
@functools.lru_cache(maxsize=None)
def _edge(count):
    from tests.test_sw import _edge as sw_edge

    q, types, rc_ab, c, _ = sw_edge(count)
    box6, mask = LJ_BOXES["xyz"]
    tab = _tabs("typed3")[0]
    ref = tf_reference(q, box6, mask, tab, lj_pairs(q, box6, mask, R_MAX * (1 + 2.0 ** -16)), types=types, rc_ab=rc_ab(3.4))
    return q, types, rc_ab, c, ref


def test_the_edge_inputs():
    """64 partners: everything finite; 65: the centre, its 65 partners and the totals NaN, everybody else finite."""
    q, types, _, c, ref = _edge(64)
    assert ref["near"][c] == 64 and ref["near"].max() == 64 and np.isfinite(ref["want"]).all() and np.isfinite(ref["ww"]).all()
    q, types, _, c, ref = _edge(65)
    assert ref["near"][c] == 65 and np.sort(ref["near"])[-2] < 64
    bad = np.isnan(ref["want"]).any(axis=1)
    assert bad.sum() == 66 and bad[c] and np.isnan(ref["want"][bad]).all() and np.isnan(ref["ww"]).all()
    assert (~bad).sum() > N // 2 and np.isfinite(ref["S"]).all()


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _set_tab(nl, tab):
    nl.set_pair_table(tab.F if tab.nt_pair > 1 else tab.F[0], tab.U if tab.nt_pair > 1 else tab.U[0], tab.r_min, tab.r_max)
    nl.set_tersoff(*tab.set_args())


def _set(nl, kind, rc, **kw):
    """The type table (three types, at the list's cut-off), the pair table and the Tersoff tables onto an initialised handle."""
    tab, types, rc_ab = _tabs(kind, **kw)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    _set_tab(nl, tab)
    return tab


def _built(q, box, dtype, rc, kind, off=0, stride=4, exclusions=None, types=None, tab=None, rc_ab=None, **kw):
    """(handle, device positions) after one full-list build, the tables set.  types: another type table than the kind's; tab: other
    tables (with rc_ab, the cut-offs of their types)."""
    torch = _torch()
    nl = _handle(box, dtype, True, rc, off)
    nl.Initialize(len(q))
    if tab is None:
        _set(nl, kind, rc, **kw)
        if types is not None:
            nl.set_type_cutoffs(types, _tabs(kind)[2](rc))
    else:
        if types is not None:
            nl.set_type_cutoffs(types, rc_ab)
        _set_tab(nl, tab)
    if exclusions is not None:
        nl.set_exclusions(exclusions, len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


def _lds_expected(tab, dtype):
    size = np.dtype(dtype).itemsize
    radial = tab.u.size * (2 if tab.p is None else 3)
    return (radial + tab.F.size) * 4 * size + (tab.nt ** 3 + tab.nt ** 2) * 4 * size + 4 * 64 * (3 * size + 4) <= 65280


def _check(f, w, ref, dtype, rows=None):
    """Forces, pe_i and the totals within their bounds; returns them on the host."""
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, ref["want"], ref["S"], dtype)[slice(None) if rows is None else rows].max(axis=0).round(2),
          virial_ratio(w, ref["ww"], ref["SW"], dtype).round(3))
    check_lj(f, ref["want"], ref["S"], dtype, c=TERSOFF_C, rows=rows)
    if rows is None:
        check_virial(w, ref["ww"], ref["SW"], dtype, c=TERSOFF_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (TERSOFF_C + TERSOFF_CW) * lj_unit(dtype) * ref["SW"][6]
    return f, w


TF = contract.Consumer(
    forces="tersoff_forces", virial="tersoff_virial", scratch="tersoff_virial", clear="clear_tersoff", info="get_tersoff",
    entry=("nl_tersoff_forces", "nl_tersoff_forces_enqueue", "nl_tersoff_virial", "nl_tersoff_virial_enqueue"), set=_set, kinds=KINDS,
    ref=_ref, moved_ref=_moved_ref, extra=lambda nl: (), check=lambda f, w, x, ref, dtype, rows=None: _check(f, w, ref, dtype, rows),
    half_lists=False, local_slabs=False)
_run = functools.partial(contract.run, TF)


def _assert_nan_pattern(f, w, ref, dtype):
    """NaN exactly where the reference has it; everybody else within the bound; all 8 totals NaN."""
    f, w = f.cpu().numpy(), w.cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,) and np.isnan(ref["ww"]).all()
    assert np.array_equal(np.isnan(f), np.isnan(ref["want"]))
    clean = ~np.isnan(ref["want"]).any(axis=1)
    if clean.any():
        check_lj(f, ref["want"], ref["S"], dtype, c=TERSOFF_C, rows=clean)


gpu = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, dtype):
    """Every box, mask and position state x "one" and "typed3" x dtype; the list cut-off, the offset width and q_stride rotate
    through the cases."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, kind in enumerate(KINDS):
        k = case + p
        rc, off, stride = (2.5, 3.4)[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        nl, qd = _built(q, box, dtype, rc, kind, off, stride)
        tab = _tabs(kind)[0]
        assert nl.get_tersoff() == dict(ntypes=tab.nt, nknots=NK, r_min=R_MIN, r_max=R_MAX, p=kind == "typed3", lds=_lds_expected(tab, dtype))
        assert nl.get_tersoff()["lds"] == (kind == "one" and dtype == np.float32)
        _run(nl, qd, _ref(box, drift, kind), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["bond short", "pair short"])
def test_second_ranges(which, dtype):
    """r_max_3 = 2.2 under a pair table to 2.5, and the other way round: n_in is exactly the pairs within the longer range."""
    box, drift = "tilt", True
    kw = {"bond short": dict(r_max_3=R_22), "pair short": dict(r_max_pair=R_22)}[which]
    for kind in KINDS:
        ref = _refs(_input(box, drift), box, kind, _pairs(box, drift), **kw)
        assert ref["ww"][7] == _ref(box, drift, kind)["ww"][7] and np.isfinite(ref["want"]).all()
        assert (ref["near"].max() < 35) == (which == "bond short")
        nl, qd = _built(_input(box, drift), box, dtype, 2.5, kind, **kw)
        _run(nl, qd, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype,lds", [(np.float32, True), (np.float64, False)])
def test_reproducible_totals_and_both_paths(dtype, lds, monkeypatch):
    """tersoff_virial twice: the same bytes.  LDS against global memory on one list: the totals bit for bit, the forces (atomics)
    within the bound, the path asserted through nl_get_tersoff.  fp32 at 3 x 1024 knots is staged (48 KiB, the parameters and the
    strips), fp64 takes the global path by size; NL_TABLE_LDS=0 around set_tersoff switches the staged one."""
    box, drift, kind = "tilt", True, "one"
    q, ref = _input(box, drift), _ref(box, drift, kind)
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nl, qd = _built(q, box, dtype, 3.4, kind)
    assert nl.get_tersoff()["lds"] == lds
    fa, wa = _run(nl, qd, ref, dtype)
    assert nl.tersoff_virial(qd).cpu().numpy().tobytes() == wa.tobytes() and len(wa.tobytes()) == 64
    monkeypatch.setenv("NL_TABLE_LDS", "0")
    nl.set_tersoff(*_tabs(kind)[0].set_args())  # (the same tables, the same list)
    assert not nl.get_tersoff()["lds"]
    fb, wb = _run(nl, qd, ref, dtype)
    assert wa.tobytes() == wb.tobytes()
    assert np.all(np.abs(fa.astype(np.float64) - fb) <= 2 * TERSOFF_C * lj_unit(dtype) * ref["S"])


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_u_is_the_pair_table(kind, dtype):
    """u = U = 0: on one full list tersoff_forces is table_forces byte for byte, pe_i included, and the totals are table_virial's."""
    box, drift = "xyz", True
    nl, qd = _built(_input(box, drift), box, dtype, 3.4, kind, bond=False)
    f, w = nl.tersoff_forces(qd).cpu().numpy(), nl.tersoff_virial(qd).cpu().numpy()
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert np.isfinite(f).all() and np.abs(f).max() > 0.1
    assert f.tobytes() == ft.tobytes() and w.tobytes() == wt.tobytes()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_pair_table(dtype):
    box, drift, kind = "tilt", False, "typed3"
    q = _input(box, drift)
    ref = _refs(q, box, kind, _pairs(box, drift), pair=False)
    assert np.array_equal(ref["want"], ref["bond"]) and np.abs(ref["want"][:, :3]).max() > 1 and ref["ww"][7] > N
    nl, qd = _built(q, box, dtype, 3.4, kind, pair=False)
    _run(nl, qd, ref, dtype)


@functools.lru_cache(maxsize=None)
def _sum_tab(nk=NK):
    """One type, u symmetric by construction: the tables of "one" with beta = 0, and the pair table phi + u (on the same grid)."""
    tab = _tabs("one", beta=False)[0]
    return tab, tab.F[0] + tab.Uu[0], tab.U[0] + tab.u[0]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_beta_is_the_pair_table_of_phi_plus_u(dtype):
    """beta = 0: b = 1 and b' = 0, so the potential is the pair potential phi + u (a full list counts every bond from both ends):
    tersoff_forces and tersoff_virial agree with table_forces and table_virial of that table within the two bounds."""
    box, drift = "xyz", False
    q = _input(box, drift)
    tab, Fs, Us = _sum_tab()
    ref = _refs(q, box, "one", _pairs(box, drift), beta=False)
    assert np.all(ref["b"] == 1.0)
    nl, qd = _built(q, box, dtype, 2.5, "one", beta=False)
    f, w = _run(nl, qd, ref, dtype)
    nl.set_pair_table(Fs, Us, R_MIN, R_MAX)
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    from tests.util_table import TABLE_C, TABLE_CW
    assert np.all(np.abs(f.astype(np.float64) - ft) <= (TERSOFF_C + TABLE_C) * lj_unit(dtype) * ref["S"])
    assert np.all(np.abs(w[:7] - wt[:7]) <= (TERSOFF_CW + TABLE_CW) * lj_unit(dtype) * ref["SW"]) and w[7] == wt[7]


@functools.lru_cache(maxsize=None)
def _dimers(count=500):
    """500 isolated dimers of three types on a grid of spacing 5.25 in the open box, r between 0.95 and 1.8 (inside f_C's ramp for
    most): (q, types, reference).  Pairs of types (0, 2) are not in the list."""
    rng = np.random.default_rng(17)
    g = np.stack(np.meshgrid(*(np.arange(8),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:count]
    mid = (g + 0.5) * 5.25
    u = rng.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = rng.uniform(0.95, 1.8, size=count)
    q = np.zeros((2 * count, 4))
    q[0::2, :3], q[1::2, :3] = mid - 0.5 * r[:, None] * u, mid + 0.5 * r[:, None] * u
    q[:, :3] = q[:, :3].astype(np.float32)
    types = rng.integers(0, 3, size=2 * count).astype(np.int32)
    box6, mask = (42.0, 42.0, 42.0, 0.0, 0.0, 0.0), 0
    tab, _, rc_ab = _tabs("typed3")
    ref = tf_reference(q, box6, mask, tab, lj_pairs(q, box6, mask, R_MAX), types=types, rc_ab=rc_ab(2.5))
    return q, types, ref


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolated_dimers(dtype):
    """zeta = 0, b = 1: the force is the plain pair force of phi + u of the slot (t_i, t_j), the energy phi + (u_ij + u_ji) / 2."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    q, types, ref = _dimers()
    tab, _, rc_ab = _tabs("typed3")
    assert np.all(ref["b"] == 1.0) and np.all(ref["zeta"] == 0.0) and ref["near"].max() == 1 and (ref["near"] == 1).sum() > 700
    I, J, d, r2 = ref["entries"]
    from md_neighbor_list_amd import rdf
    fr = np.zeros(len(I))
    for k in range(len(I)):  # the pair force, written out
        a, b = int(types[I[k]]), int(types[J[k]])
        s = rdf.slot(a, b, 3)
        fr[k] = pair_table.interpolate(tab.F[s], tab.U[s], R_MIN, R_MAX, r2[k:k + 1])[0][0]
        fr[k] += 0.5 * (pair_table.interpolate(tab.Uu[a * 3 + b], tab.u[a * 3 + b], R_MIN, R_MAX, r2[k:k + 1])[0][0] +
                        pair_table.interpolate(tab.Uu[b * 3 + a], tab.u[b * 3 + a], R_MIN, R_MAX, r2[k:k + 1])[0][0])
    plain = np.zeros((len(q), 3))
    np.add.at(plain, I, fr[:, None] * d)
    assert np.allclose(plain, ref["want"][:, :3], rtol=1e-12, atol=1e-12)
    nl = NeighListGPU(2.5, 42.0, 42.0, 42.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=True, minimum_image=False)
    nl.Initialize(len(q))
    nl.set_type_cutoffs(types, rc_ab(2.5))
    _set_tab(nl, tab)
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, len(q))
    _run(nl, qd, ref, dtype)


def _trimers(dtype, count=300):
    """Isolated symmetric trimers, two types: a centre of type 1 with two ends of type 0 at one distance r in [1.0, 1.5] and an
    angle between 60 and 180 degrees.  Only the slot (1, 0) has a u; every other u is 0, so the per-particle energy of an end is
    b u / 4 of its one bond and nothing else.  Returns (q, types, tables, centre of every end, the other end of every end)."""
    rng = np.random.default_rng(23)
    g = np.stack(np.meshgrid(*(np.arange(7),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:count]
    mid = (g + 0.5) * 6.0
    r = rng.uniform(1.0, 1.5, size=count)
    th = rng.uniform(np.pi / 3, np.pi, size=count)
    q = np.zeros((3 * count, 4))
    q[0::3, :3] = mid
    q[1::3, :3] = mid + r[:, None] * np.array([1.0, 0.0, 0.0])
    q[2::3, :3] = mid + r[:, None] * np.stack([np.cos(th), np.sin(th), np.zeros(count)], axis=1)
    q[:, :3] = q[:, :3].astype(np.float32)
    types = np.zeros(3 * count, dtype=np.int32)
    types[0::3] = 1
    u, Uu, qq, Qq, _, _ = _radial(2, False, R_MIN, R_MAX, NK)
    keep = np.zeros((4, 1))
    keep[2] = 1.0  # the slot (1, 0)
    gam, c2d2, d2, h, _, _ = tf_parameters(2)
    beta, n = tersoff.bond_order(np.full((2, 2), 3.0), np.array([[2.5, 2.2], [0.8, 2.5]]))
    F0 = np.zeros(NK)
    tab = TfTables(F0, F0, R_MIN, R_MAX, u * keep, Uu * keep, qq, Qq, None, None, R_MIN, R_MAX, 10.0 * gam, c2d2, d2, h, beta, n)
    ends = np.sort(np.concatenate([np.arange(count) * 3 + 1, np.arange(count) * 3 + 2]))
    return q, types, tab, ends // 3 * 3, np.where(ends % 3 == 1, ends + 1, ends - 1), ends


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolated_trimers_recover_b(dtype):
    """b recovered from the energy of an end, 4 pe_j / u_j, against b of the exact powers of the SAME t = beta zeta: with one
    other partner zeta_j = g_jk q_k is a single product, so everything in front of the two pow is followed bit for bit in T here
    (positions, a, r2, the knots, cs, g, zeta, t).  What is left is: tn within P ulp, its part s / (2 n) of b, the rounding of
    1 + tn, b within P ulp and the rounding of b u -- P = POW_ULP, the accuracy the header assumes of pow.  Prints the largest
    deviation in ulp of b (DESIGN.md section 8y records it)."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    T = np.dtype(dtype).type
    q, types, tab, centre, other, ends = _trimers(dtype)
    p = q[:, :3].astype(T)
    a, bv = p[centre] - p[ends], p[centre] - p[other]
    r2a, r2b = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2], (bv[:, 0] * bv[:, 0] + bv[:, 1] * bv[:, 1]) + bv[:, 2] * bv[:, 2]
    UUt, dUUt, ut, dut, x0, xc, iD = table_device_form(tab.Uu, tab.u, R_MIN, R_MAX, T)
    QQt, dQQt, qt, dqt = table_device_form(tab.Qq, tab.q, R_MIN, R_MAX, T)[:4]
    slot = np.full(len(ends), 2)
    ia, ba, ka, ta = _knot(r2a, x0, xc, iD, NK, T)
    ib, bb, kb, tb = _knot(r2b, x0, xc, iD, NK, T)
    uj, qk = _lin(ut, dut, slot, ka, ta, ia, ba, T), _lin(qt, dqt, slot, kb, tb, ib, bb, T)
    ira, irb = T(1) / np.sqrt(r2a), T(1) / np.sqrt(r2b)
    cs = (((a[:, 0] * bv[:, 0] + a[:, 1] * bv[:, 1]) + a[:, 2] * bv[:, 2]) * ira) * irb
    gam, gc, d2, h = (v[1, 0, 0] for v in (tab.ang[0].astype(T), (tab.ang[0] * tab.ang[1]).astype(T), tab.ang[2].astype(T), tab.ang[3].astype(T)))
    x = h - cs
    x2 = x * x
    zeta = T(1) * ((gam + gc * (x2 / (d2 + x2))) * qk)
    beta, n = tab.beta.astype(T)[1, 0], tab.n.astype(T)[1, 0]
    e2 = T(-1.0 / (2.0 * tab.n[1, 0]))
    t = beta * zeta
    assert t.dtype == np.dtype(T) and np.all(zeta > 0) and np.all(uj < 0)
    L = np.longdouble
    tn = t.astype(L) ** L(n)
    b_exact = (L(1) + tn) ** L(e2)
    s = np.asarray(tn / (1 + tn), dtype=np.float64)
    print("b between", float(b_exact.min()), float(b_exact.max()))
    assert b_exact.min() < 0.3 and b_exact.max() > 0.85  # (the whole bend of b)
    nl = NeighListGPU(2.5, 42.0, 42.0, 42.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=True, minimum_image=False)
    nl.Initialize(len(q))
    nl.set_type_cutoffs(types, np.full((2, 2), 2.5))
    _set_tab(nl, tab)
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, len(q))
    f = nl.tersoff_forces(qd).cpu().numpy()
    b_got = (4.0 * f[ends, 3].astype(L)) / uj.astype(L)
    ulp = np.spacing(np.asarray(b_exact, dtype=T)).astype(np.float64)
    dev = np.asarray(np.abs(b_got - b_exact), dtype=np.float64) / ulp
    # tn: P ulp of it; 1 + tn: half an ulp; both reach b scaled by s / (2 n) (and at most doubled by the ulp of b against that of
    # tn or 1 + tn); then P ulp of b itself and half an ulp of b u
    allowed = POW_ULP + 0.5 + 2.0 * (POW_ULP + 0.5) * s / (2.0 * float(n)) * 2.0
    print(np.dtype(dtype).name, "largest deviation of b in ulp:", dev.max().round(3), "allowed there", allowed[int(np.argmax(dev))].round(3))
    assert np.all(dev <= allowed)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [64, 65])
def test_the_64_partner_edge(count, dtype):
    """A centre with exactly 64 partners in range is finite and within the bound; with 65, the centre, its 65 partners and all 8
    totals are NaN, every other particle is within the bound and the NaN pattern is the reference's."""
    q, types, rc_ab, c, ref = _edge(count)
    nl, qd = _built(q, "xyz", dtype, 2.5, "typed3", types=types)
    f, w = nl.tersoff_forces(qd), nl.tersoff_virial(qd)
    if count == 64:
        assert np.isfinite(f[c].cpu().numpy()).all()
        _check(f, w, ref, dtype)
    else:
        assert np.isnan(f[c].cpu().numpy()).all()
        _assert_nan_pattern(f, w, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_partner_below_the_radial_tables(dtype):
    """One particle moved to 0.5 from its neighbour: below r_min_3 = 0.85, inside the pair table (sampled from 0.4 here).  Both are
    centres with a partner below the tables: NaN for them and all their partners in range, and in all 8 totals."""
    box, kind = "xyz", "one"
    box6, mask = LJ_BOXES[box]
    q = _input(box, False).copy()
    a = int(np.ravel_multi_index((6, 7, 5), (LJ_M,) * 3))
    b = int(np.ravel_multi_index((7, 7, 5), (LJ_M,) * 3))
    q[b, :3] = (q[a, :3] + [0.5, 0.0, 0.0]).astype(np.float32)
    pairs = lj_pairs(q, box6, mask, R_MAX * (1 + 2.0 ** -16))
    r2 = (pairs[2] ** 2).sum(axis=1)
    for cut in (0.4, R_MIN, R_MAX):
        assert not np.any(np.abs(r2 / cut ** 2 - 1.0) < 2.0 ** -17)
    assert (np.sqrt(r2) < R_MIN).sum() == 2
    ref = _refs(q, box, kind, pairs, r_min_pair=0.4)
    bad = np.isnan(ref["want"]).any(axis=1)
    near = np.unique(np.concatenate([pairs[1][(pairs[0] == a) | (pairs[0] == b)], [a, b]]))
    assert np.array_equal(np.flatnonzero(bad), near) and np.isnan(ref["want"][bad]).all() and 45 < bad.sum() < 100
    nl, qd = _built(q, box, dtype, 2.5, kind, r_min_pair=0.4)
    _assert_nan_pattern(nl.tersoff_forces(qd), nl.tersoff_virial(qd), ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_lone_partner_below_the_radial_tables(dtype):
    """Two isolated dimers, one at 0.5 (below r_min_3, inside the pair table): unlike Stillinger-Weber a lone partner has a bond, so
    both its particles and all 8 totals are NaN; the other dimer is within the bound."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    q = np.zeros((4, 4))
    q[:, :3] = np.array([[5.0, 5.0, 5.0], [5.5, 5.0, 5.0], [15.0, 15.0, 15.0], [15.0, 16.25, 15.0]])
    box6, mask = (21.0, 21.0, 21.0, 0.0, 0.0, 0.0), 0
    tab = _tabs("one", r_min_pair=0.4)[0]
    ref = tf_reference(q, box6, mask, tab, lj_pairs(q, box6, mask, R_MAX))
    assert np.isnan(ref["want"][:2]).all() and np.isfinite(ref["want"][2:]).all() and np.abs(ref["want"][2:, :3]).max() > 0.01
    nl = NeighListGPU(2.5, 21.0, 21.0, 21.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=True, minimum_image=False)
    nl.Initialize(4)
    _set_tab(nl, tab)
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, 4)
    _assert_nan_pattern(nl.tersoff_forces(qd), nl.tersoff_virial(qd), ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_exclusions(dtype):
    """A list filtered by nl_set_exclusions (the bonds along x): an excluded partner forms no pair term, no bond and enters no
    zeta; the unfiltered reference is refused."""
    box, kind = "xyz", "one"
    q = _input(box, False)
    ref = _refs(q, box, kind, _pairs(box, False), exclusions=_bonds())
    assert ref["near"].max() <= 47 and ref["ww"][7] == _ref(box, False, kind)["ww"][7] - N
    nl, qd = _built(q, box, dtype, 2.5, kind, exclusions=_bonds())
    f, _ = _run(nl, qd, ref, dtype)
    with pytest.raises(AssertionError):
        check_lj(f, _ref(box, False, kind)["want"], ref["S"], dtype, c=TERSOFF_C)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,kind", [("xyz", "one"), ("tilt", "typed3")])
def test_reuse_within_the_skin(box, kind, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants; no extra build."""
    contract.reuse_within_the_skin(TF, box, kind, True, dtype)


@gpu
def test_captured():
    """A capture of tersoff_virial before its first call is NL_ERR_STATE (the scratch cannot be allocated); after one synchronous
    call one graph holds the copy of the positions, the update, the forces and the totals, replayed at two position sets."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()

    def before(nl, qd, fd, wd):
        nl.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0):
            with pytest.raises(NLError) as e:
                nl.tersoff_virial(qd, wait=False, out=wd)
            assert e.value.code == NL_ERR_STATE
            nl.tersoff_forces(qd, wait=False, out=fd)  # (the forces need no scratch)
        nl.tersoff_virial(qd)  # synchronous, outside a capture: allocates

    contract.captured(TF, True, before, lambda nl, replay: None)  # (nothing is set afterwards)


def _wide_tab(r_max_3, r_min=1e-3):
    """The one-type Tersoff arguments on a grid from r_min (a uniform random box has close pairs) to r_max_3."""
    u, Uu, q, Qq, _, _ = _radial(1, False, r_min, r_max_3, NK)
    return (u, Uu, q, Qq, r_min, r_max_3) + tuple(tf_parameters(1))


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces and totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat all are finite."""
    def set_tables(nl):
        nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, R_MAX, NK), 1e-3, R_MAX)
        nl.set_tersoff(*_wide_tab(1.5))  # (about 13 partners within 1.5)

    def prepare(nl, qd):
        nl.update(qd, sync=True)
        nl.tersoff_virial(qd)  # (the scratch)

    contract.failed_list(TF, set_tables, prepare)


@gpu
@pytest.mark.parametrize("off", [32, 64])
def test_both_offset_widths(off):
    contract.both_offset_widths(TF, True, off)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_on_a_callers_held_stream(dtype):
    """A non-blocking stream of the caller's, held back by a delay: the positions are written behind the delay, and the update,
    the forces and the totals enqueued on that stream read what was written."""
    from tests.consumer_util import _tdt
    from tests.stream_util import device, held_stream, rolled

    torch = _torch()
    box, kind = "xyz", "one"
    q = _input(box, False)
    nl = _handle(box, dtype, True, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    _set(nl, kind, 2.9)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    qd = dec.clone()
    fd = torch.empty((N, 4), dtype=_tdt(dtype), device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    nl.update(qd, sync=True)  # (warm, on the decoy: nothing allocates while the stream is held)
    nl.tersoff_forces(qd, wait=False, out=fd), nl.tersoff_virial(qd, wait=False, out=wd)
    nl.tersoff_virial(qd)
    torch.cuda.synchronize()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        nl.tersoff_forces(qd, wait=False, out=fd), nl.tersoff_virial(qd, wait=False, out=wd)
        h.assert_held(f"tersoff {np.dtype(dtype).name}")
    nl.synchronize()
    _check(fd, wd, _ref(box, False, kind), dtype)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    tab, _, _ = _tabs("one")
    tab3, types, rc_ab = _tabs("typed3")
    F, U = tab.F[0], tab.U[0]
    q = _input("open", False)
    nl = _handle("open", np.float32, True, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    calls = contract.entry_calls(TF, lib, fd, out)
    set_one = lambda t=tab: nl.set_tersoff(*t.set_args())  # noqa: E731
    # nothing set; only the pair table; only the Tersoff tables
    assert nl.get_tersoff() is None and lib.nl_get_tersoff(nl._h, *([None] * 6)) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for have_pair, have_tf in ((False, False), (True, False), (False, True)):
        nl.set_pair_table(F, U, R_MIN, R_MAX) if have_pair else nl.clear_pair_table()
        set_one() if have_tf else nl.clear_tersoff()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    want = nl.tersoff_virial(qd).cpu().numpy()
    assert np.isfinite(want).all()
    # the setter's arguments: each refused, and the tables that were set are kept
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    names = ("u", "U", "q", "Q", "p", "P", "gamma", "c2d2", "d2", "h", "beta", "n")
    good = dict(nt=1, nk=NK, lo=R_MIN, hi=R_MAX, u=tab.u[0], U=tab.Uu[0], q=tab.q[0], Q=tab.Qq[0], p=None, P=None, gamma=tab.ang[0], c2d2=tab.ang[1],
                d2=tab.ang[2], h=tab.ang[3], beta=tab.beta, n=tab.n)
    keep = []  # (the arrays behind the pointers)

    def args(**kw):
        a = dict(good, **kw)
        ptrs = {k: None if a[k] is None else dp(a[k]) for k in names}
        keep.append(ptrs)
        return (a["nt"], a["nk"], a["lo"], a["hi"]) + tuple(ptrs[k] for k in names)

    bad_u, bad_Q = tab.u[0].copy(), tab.Qq[0].copy()
    bad_u[5], bad_Q[7] = np.inf, np.nan
    big = np.zeros(4097)
    one = np.ones(NK)
    typed5 = dict(nt=5, u=np.zeros((25, NK)), U=np.zeros((25, NK)), q=np.zeros((25, NK)), Q=np.zeros((25, NK)), gamma=np.ones(125), c2d2=np.ones(125),
                  d2=np.ones(125), h=np.zeros(125), beta=np.ones(25), n=np.ones(25))
    for kw in (dict(u=None), dict(U=None), dict(q=None), dict(Q=None), dict(gamma=None), dict(c2d2=None), dict(d2=None), dict(h=None), dict(beta=None),
               dict(n=None), dict(p=one), dict(P=one), dict(nk=1), dict(nk=-2), dict(nk=4097, u=big, U=big, q=big, Q=big), dict(lo=0.0), dict(lo=-1.0),
               dict(lo=R_MAX), dict(hi=np.inf), dict(lo=np.nan), dict(nt=0), typed5, dict(u=bad_u), dict(Q=bad_Q), dict(p=bad_u, P=one),
               dict(d2=np.array([0.0])), dict(d2=np.array([-1.0])), dict(d2=np.array([np.nan])), dict(n=np.array([0.0])), dict(n=np.array([-2.0])),
               dict(n=np.array([np.inf])), dict(beta=np.array([-1e-9])), dict(beta=np.array([np.nan])), dict(gamma=np.array([np.inf])),
               dict(c2d2=np.array([np.nan])), dict(h=np.array([np.inf]))):
        assert lib.nl_set_tersoff(nl._h, *args(**kw)) == NL_ERR_ARG, kw.keys()
        assert nl.get_tersoff()["nknots"] == NK and nl.get_tersoff()["ntypes"] == 1 and not nl.get_tersoff()["p"]
    assert lib.nl_set_tersoff(None, *args()) == NL_ERR_ARG
    assert lib.nl_set_tersoff(nl._h, *args(p=one, P=one)) == 0 and nl.get_tersoff()["p"]
    assert lib.nl_set_tersoff(nl._h, *args(beta=np.array([0.0]))) == 0 and not nl.get_tersoff()["p"]
    set_one()
    assert nl.tersoff_virial(qd).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(TypeError):
        nl.set_tersoff(tab.u[0], tab.Uu[0][:-1], tab.q[0], tab.Qq[0], R_MIN, R_MAX, *tab.ang, tab.beta, tab.n)
    with pytest.raises(TypeError):
        nl.set_tersoff(tab3.u, tab3.Uu, tab3.q, tab3.Qq, R_MIN, R_MAX, *tab.ang, tab.beta, tab.n)  # 9 slots, one triple
    with pytest.raises(TypeError):
        nl.set_tersoff(*tab.set_args()[:-2], p=one)  # p without P
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_one)
    # reach of the radial tables (the pair table stays at 2.5); from 2.7 on some centres have more than 64 partners in range
    contract.reach(TF, nl, qd, lambda r_max: nl.set_tersoff(*_wide_tab(r_max, R_MIN)))
    # ... and of the pair table
    set_one()
    nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, 2.7, NK), R_MIN, 2.7)
    nl.tersoff_forces(qd)
    with pytest.raises(NLError) as e:
        nl.tersoff_forces(qd, wait=False)
    assert e.value.code == NL_ERR_ARG
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    contract.clearing(TF, nl, qd, set_one, lambda: lib.nl_set_tersoff(nl._h, *args(nk=0)))
    set_one()
    assert lib.nl_set_tersoff(nl._h, 1, NK, R_MIN, R_MAX, *([None] * 12)) == 0 and nl.get_tersoff() is None  # all NULL clears
    # several types: a type table of that ntypes, a pair table of 1 or ntypes types
    contract.several_types(TF, nl, qd, types, set_one, lambda: set_one(tab3))  # (a pair table of one type under nine slots)
    nl.set_pair_table(tab3.F, tab3.U, R_MIN, R_MAX)
    assert torch.isfinite(nl.tersoff_forces(qd)).all()
    # a half list
    half = _handle("open", np.float32, False, 2.9)
    half.Initialize(N)
    _set_tab(half, tab)
    half.MakeNeighList(qd, N)
    assert torch.isfinite(half.table_forces(qd)).all()  # (the pair table's calls take this list)
    for fn, o in calls:
        assert fn(half._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    contract.no_particles(TF, lib, True, lambda empty: _set_tab(empty, tab), qd, fd, out)


@gpu
def test_slab_lists_are_refused():
    """A full-list slab build, with and without nl_set_local_ids: NL_ERR_STATE from all four calls."""
    contract.slab_lists_are_refused(TF, True)


@gpu
def test_distributed_lists_are_refused():
    """A distributed build of a world of one: its list holds caller ids, and all four calls are NL_ERR_STATE, wait and enqueue."""
    contract.distributed_lists_are_refused(TF, True)

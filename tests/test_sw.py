"""Stillinger-Weber three-body potentials (nl_set_sw, nl_sw_forces, nl_sw_virial and their enqueue variants) against a
float64 evaluation of the rule, with an error bound per particle and per component.

Contract tested (include/nl_hip.h, nl_set_sw):
  * |got - want| <= SW_C u S for every particle and each of fx, fy, fz, pe on its own, and <= SW_CW u S for each of the 7 sums of
    the totals, n_in exact.  want: tests.util_sw sw_reference (md_neighbor_list_amd.sw three_body and pair_table.interpolate on
    the caller's double tables over an O(N^2) pair sweep, no list).  S: the uncancelled sums over pairs and triples, built with
    |cs| + |c0| in place of |dc| (dc can vanish) and with the three terms of every table read, which carry the conditioning of
    the read on the rounding of its r^2;
  * NaN rules (more than 64 partners in range, a partner below the radial table), LDS against global, reproducible totals, the
    enqueue variants, state and arguments.

The constants are not fitted to the kernel.  Each is 4 x the largest ratio that a numpy emulation of the stated rule in the
position type reaches against the float64 reference (tests.util_sw sw_emulate: one rounding per operation, no FMA, random
summation orders, knots and scalars rounded as the setters round them; the totals with the kernels' summation tree) over the
inputs of EMULATED, in float32 and in float64; test_emulation_gives_c recomputes them.  The factor 4 covers the GPU's other
summation order.  Because dc can vanish no weakest term bounds the result from below: sharpness is shown by the defects of
test_wrong_results_are_rejected.

The inputs are those of tests/test_pair_table.py: the 14^3 jittered lattice, n = 2744, on the boxes of LJ_BOXES, in the box and
drifted, and _moved.  The radial tables live on the pair table's grid (R_MIN, R_MAX = 2.5), with 2.2 and 1.8 as second ranges
(test_inputs: the partner counts and the bands).  The test g is the Stillinger-Weber radial form with a sigma = 3.2 beyond the
table's end, so it does not vanish at r_max_3 and a dropped partner is visible.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import pair_table, sw
from tests import consumer_contract as contract
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _bonds, _handle, _pair_tab, _tab, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_A, LJ_BOXES, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_unit
from tests.util_sw import (A_SIGMA, DEFECTS, SW_C, SW_CW, SwTables, sw_angular, sw_emulate, sw_energy, sw_functions, sw_reference)
from tests.util_table import morse
from tests.virial_util import check_virial, virial_ratio

KINDS = ("one", "three")
R_22, R_18 = 2.2, 1.8  # the second ranges
EMULATED = [("open", False, "one"), ("xyz", False, "one"), ("tilt", True, "one"), ("xyz", True, "three"), ("tilt", False, "three"),
            ("open", False, "three")]
EMULATED_MAX, EMULATED_MAX_W = 0.51, 0.0635  # the largest ratios of test_emulation_gives_c: per particle, and of the totals


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _tabs(kind, nk=NK, r_max_3=R_MAX, r_max_pair=R_MAX, r_min_pair=R_MIN, r_min_3=R_MIN, pair=True, three=True):
    """(SwTables, types, rc_ab(rc_list)) of a potential: one type with the Morse table, or the 3-type mixture of test_pair_table's
    typed3, whose pair (0, 2) the type table leaves out of the list, with a g slot per ordered pair of types and Lambda, c0 per
    triple.  pair=False: a zero pair table; three=False: Lambda = 0."""
    nt = 1 if kind == "one" else 3
    F, U, types, rc_ab = _tab("morse" if nt == 1 else "typed3", nk)
    if (r_min_pair, r_max_pair) != (R_MIN, R_MAX):
        F, U = _pair_tab(nt, r_min_pair, r_max_pair, nk)
    gs, dgs = sw_functions(nt)
    g, G = sw.sample(gs, dgs, r_min_3, r_max_3, nk) if nt > 1 else sw.sample(gs[0][0], dgs[0][0], r_min_3, r_max_3, nk)
    lam, c0 = sw_angular(nt)
    if not three:
        lam = np.zeros_like(lam)
    if not pair:
        F, U = np.zeros_like(F), np.zeros_like(U)
    return SwTables(F, U, r_min_pair, r_max_pair, g, G, r_min_3, r_max_3, lam, c0), types, rc_ab


def _refs(q, box, kind, pairs, exclusions=None, **kw):
    box6, mask = LJ_BOXES[box]
    tab, types, rc_ab = _tabs(kind, **kw)
    return sw_reference(q, box6, mask, tab, pairs, types=types, rc_ab=None if rc_ab is None else rc_ab(3.4), exclusions=exclusions)


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
    assert int(re.search(r"#define NL_SW_MAX_TYPES\s+(\d+)", text).group(1)) == 4 == sw.MAX_TYPES
    assert int(re.search(r"#define NL_SW_MAX_NEAR\s+(\d+)", text).group(1)) == 64 == sw.MAX_NEAR
    assert int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1)) == 65280
    for name in ("nl_set_sw", "nl_get_sw", "nl_sw_forces", "nl_sw_forces_enqueue", "nl_sw_virial", "nl_sw_virial_enqueue"):
        assert re.search(r"\bint %s\(" % name, text), name


def test_inputs():
    """What the issue measured of the inputs: the most partners of any centre within 2.5 is 49 (48 for the moved ones), within
    2.2 it is 31 and within 1.8 it is 22; about 2.4 M triples per input at 2.5; no pair within 2^-17 (relative, r^2) of 1.8 or
    2.2; the smallest distance is 0.932 (0.887 among the moved ones), above R_MIN.  The test g does not vanish at the end of any table."""
    most = {R_MAX: 0, R_22: 0, R_18: 0}
    closest = 9.0
    sets = [(_pairs(box, drift), False) for box, drift in CASES] + [(_moved(box)[1], True) for box in ("xyz", "tilt")]
    most_moved = 0
    for pairs, moved in sets:
        I, _, d, _ = pairs
        r2 = (d * d).sum(axis=1)
        assert np.sqrt(r2.min()) > R_MIN + 0.03
        if not moved:
            closest = min(closest, np.sqrt(r2.min()))
        for cut in (R_22, R_18):
            assert not np.any(np.abs(r2 / cut ** 2 - 1.0) < 2.0 ** -17)
        for cut in most:
            m = np.bincount(I[r2 < cut * cut], minlength=N).max()
            if moved and cut == R_MAX:
                most_moved = max(most_moved, m)
            else:
                most[cut] = max(most[cut], m)
    print(most, most_moved, closest)
    assert most == {R_MAX: 49, R_22: 31, R_18: 22} and most_moved == 48 and most[R_MAX] < sw.MAX_NEAR
    assert 0.93 < closest < 0.935 and closest > R_MIN
    assert 2.3e6 < _ref("xyz", False, "one")["triples"] < 2.5e6
    for kind in KINDS:
        for r3 in (R_MAX, R_22, R_18):
            tab = _tabs(kind, r_max_3=r3)[0]
            assert np.all(tab.g[:, -1] > 0.1) and np.all(tab.G[:, -1] > 0.1)
    tab, types, rc_ab = _tabs("three")
    assert tab.g.shape == (9, NK) and not np.allclose(tab.g[1], tab.g[3]) and rc_ab(3.4)[0, 2] == 0  # slot (0, 1) is not slot (1, 0)
    assert len(np.unique(tab.lam)) >= 14 and np.array_equal(tab.lam, tab.lam.transpose(0, 2, 1)) and np.abs(tab.cos0).max() < 1


def test_the_rule_in_float64():
    """three_body on a hand-made triple, and against the plain triple loop on a small cluster of two types."""
    nk = 8
    g, G = np.full(nk, 2.0), np.zeros(nk)  # g = 2 everywhere: no radial force
    I, J = np.array([0, 0, 1, 2]), np.array([1, 2, 0, 0])
    d = np.array([[-1.0, 0, 0], [0, -1.5, 0], [1.0, 0, 0], [0, 1.5, 0]])  # centre 0 at the origin, 1 on +x, 2 on +y: cs = 0
    out = sw.three_body(3, I, J, d, g, G, 0.5, 2.0, *sw.angular(3.0, 1.0, -0.5))
    h = 3.0 * 0.25 * 4.0
    assert np.allclose(out["f"][:, 3], h / 3) and np.isclose(out["u"], h) and np.array_equal(out["near"], [2, 1, 1])
    # F_1 = 2 Lambda dc g g b / (ra rb) = 12 b / 1.5 with b = (0, -1.5, 0): (0, -12, 0); F_2 = 12 a / 1.5, a = (-1, 0, 0)
    assert np.allclose(out["f"][1, :3], [0, -12.0, 0]) and np.allclose(out["f"][2, :3], [-8.0, 0, 0]) and np.allclose(out["f"][0, :3], [8.0, 12.0, 0])
    assert np.allclose(out["w"], [-(-1.0) * 0 - 0 * (-8.0), -(-1.5) * 0 - 0, 0, -((-1.0) * (-12.0)), 0, 0])
    # beyond r_max_3, and below r_min_3
    far = sw.three_body(3, I, J, 1.9 * d, g, G, 0.5, 2.0, *sw.angular(3.0, 1.0, -0.5))  # 1.9 and 2.85: one partner, no triple
    assert far["near"].tolist() == [1, 1, 0] and not far["f"].any() and far["u"] == 0
    assert sw.three_body(3, I, J, 2.0 * d, g, G, 0.5, 2.0, *sw.angular(3.0, 1.0, -0.5))["near"].tolist() == [0, 0, 0]  # r = r_max_3 is out
    low = sw.three_body(3, I, J, 0.4 * d, g, G, 0.5, 2.0, *sw.angular(3.0, 1.0, -0.5))
    assert np.isnan(low["f"]).all() and np.isnan(low["u"])
    # the triple loop, open box, two types
    rng = np.random.default_rng(2)
    grid = np.stack(np.meshgrid(*(np.arange(3),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = grid * 1.1 + rng.uniform(-0.1, 0.1, size=grid.shape)
    n = len(q)
    types = rng.integers(0, 2, size=n)
    gs, dgs = sw_functions(2)
    g2, G2 = sw.sample(gs, dgs, 0.5, 1.8, 64)
    lam, c0 = sw_angular(2)
    pairs = lj_pairs(q, (9.0, 9.0, 9.0, 0.0, 0.0, 0.0), 0, 1.8)
    out = sw.three_body(n, pairs[0], pairs[1], pairs[2], g2, G2, 0.5, 1.8, lam, c0, types=types)
    f, E = np.zeros((n, 4)), 0.0
    for i in range(n):
        near = [j for j in range(n) if j != i and ((q[i] - q[j]) ** 2).sum() < 1.8 ** 2]
        for x, j in enumerate(near):
            for k in near[x + 1:]:
                a, b = q[i] - q[j], q[i] - q[k]
                ra, rb = np.linalg.norm(a), np.linalg.norm(b)
                Ga, ga, _ = pair_table.interpolate(G2[types[i] * 2 + types[j]], g2[types[i] * 2 + types[j]], 0.5, 1.8, ra * ra)
                Gb, gb, _ = pair_table.interpolate(G2[types[i] * 2 + types[k]], g2[types[i] * 2 + types[k]], 0.5, 1.8, rb * rb)
                L, cc = lam[types[i], types[j], types[k]], c0[types[i], types[j], types[k]]
                cs = a @ b / (ra * rb)
                dc = cs - cc
                Fj = -L * dc * dc * Ga * gb * a + 2 * L * dc * ga * gb * (b / (ra * rb) - cs * a / ra ** 2)
                Fk = -L * dc * dc * Gb * ga * b + 2 * L * dc * ga * gb * (a / (ra * rb) - cs * b / rb ** 2)
                h = L * dc * dc * ga * gb
                f[j, :3] += Fj
                f[k, :3] += Fk
                f[i, :3] -= Fj + Fk
                f[[i, j, k], 3] += h / 3
                E += h
    assert np.allclose(out["f"], f, rtol=1e-12, atol=1e-12) and np.isclose(out["u"], E, rtol=1e-13)
    assert np.abs(out["f"][:, :3].sum(axis=0)).max() < 1e-11 and out["near"].max() > 8


def test_sampled_tables_converge():
    """The radial tables and the Stillinger-Weber pair table against the functions they sample, on a dense grid: the largest error
    falls 4 x per doubling of the knots."""
    gs, dgs = sw_functions(3)
    u, du = sw.pair(7.049556277, 0.6022245584, 4.0, 0.0, 1.0, 1.0, 1.8)
    x = np.linspace(0.92 ** 2, R_MAX ** 2, 100001)[:-1]
    xs = np.linspace(0.92 ** 2, 1.75 ** 2, 100001)[:-1]
    worst = []
    for nk in (256, 512, 1024, 2048):
        g, G = sw.sample(gs, dgs, R_MIN, R_MAX, nk)
        w = []
        for s, (a, b) in enumerate([(a, b) for a in range(3) for b in range(3)]):
            Gv, gv, inn = pair_table.interpolate(G[s], g[s], R_MIN, R_MAX, x)
            assert inn.all()
            w += [np.abs(gv - gs[a][b](np.sqrt(x))).max(), np.abs(Gv + dgs[a][b](np.sqrt(x)) / np.sqrt(x)).max()]
        F, U = pair_table.sample(u, du, R_MIN, 1.75, nk)
        fr, pe, _ = pair_table.interpolate(F, U, R_MIN, 1.75, xs)
        w += [np.abs(pe - u(np.sqrt(xs))).max(), np.abs(fr + du(np.sqrt(xs)) / np.sqrt(xs)).max()]
        worst.append(w)
    ratios = np.array(worst[:-1]) / np.array(worst[1:])
    print("ratios", ratios.round(2))
    assert np.all((ratios > 3.0) & (ratios < 5.0))
    g1 = sw.sample(gs[0][0], dgs[0][0], R_MIN, R_MAX, 64)
    assert g1[0].shape == (64,) and np.array_equal(g1[0], sw.sample(gs, dgs, R_MIN, R_MAX, 64)[0][0])
    gg, dg = sw.radial(1.2, 1.0, 1.8)
    assert gg(1.8) == 0 and dg(1.8) == 0 and gg(2.0) == 0 and dg(1.9) == 0 and gg(1.0) == np.exp(1.2 / (1.0 - 1.8)) and u(1.8) == 0 and du(1.81) == 0
    with pytest.raises(ValueError):
        sw.angular(np.arange(8.0).reshape(2, 2, 2), 1.0, 0.0)  # not symmetric in the ends


def test_reference_is_the_gradient_of_its_energy():
    """sw_reference's forces at 4096 knots against the central difference of the ANALYTIC energy, tilted and periodic.  The
    tolerance is the interpolation error of the tables, measured per table on a dense grid (it falls 4 x per doubling) and carried
    through the rule: per pair err_phi |d|, per end of a triple Lambda (dc^2 (err_G g_b + |G_a| err_g) |a| + 2 |dc| (g_a + g_b)
    err_g (|b| ir_a ir_b + |cs| |a| ir_a^2)); plus the truncation error of the difference."""
    rng = np.random.default_rng(3)
    m, a0 = 5, 1.125
    box6, mask = (m * a0, m * a0, m * a0, a0, -a0, 2 * a0), 7
    grid = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (grid + 0.5) * a0 + rng.uniform(-0.1, 0.1, size=grid.shape)
    r_min, r_max, nk, h = 0.5, 1.8, 4096, 1e-5
    u, du = morse()
    gf, dgf = sw.radial(1.2, 1.0, A_SIGMA)
    lam, c0 = 2.0, -1.0 / 3.0
    F, U = pair_table.sample(u, du, r_min, r_max, nk)
    g, G = sw.sample(gf, dgf, r_min, r_max, nk)
    tab = SwTables(F, U, r_min, r_max, g, G, r_min, r_max, lam, c0)
    pairs = lj_pairs(q, box6, mask, r_max)
    ref = sw_reference(q, box6, mask, tab, pairs)
    I, J, d, r2 = ref["entries"]
    assert np.abs(np.sqrt(r2) - r_max).min() > 10 * h
    x = np.linspace(0.8 ** 2, r_max ** 2, 400001)[:-1]
    rr = np.sqrt(x)
    err_phi = np.abs(pair_table.interpolate(F, U, r_min, r_max, x)[0] + du(rr) / rr).max()
    Gv, gv, _ = pair_table.interpolate(G, g, r_min, r_max, x)
    err_g, err_G = np.abs(gv - gf(rr)).max(), np.abs(Gv + dgf(rr) / rr).max()
    tb = sw.three_body(len(q), I, J, d, g, G, r_min, r_max, tab.lam, tab.cos0, parts=True)
    e, a, _, _ = tb["ends"]
    P, K, cs, cc, L, ga, gb, Ga, ira, irb = tb["tri"]
    na, nb, dc = 1.0 / ira, 1.0 / irb, np.abs(cs - cc)
    per = L * (dc * dc * (err_G * gb + np.abs(Ga) * err_g) * na + 2 * dc * (ga + gb) * err_g * (nb * ira * irb + np.abs(cs) * na * ira * ira))
    per_end = np.bincount(P, weights=per, minlength=len(e))
    tol3 = np.bincount(J[e], weights=per_end, minlength=len(q)) + np.bincount(I[e], weights=per_end, minlength=len(q))
    tol2 = np.bincount(I, weights=err_phi * np.sqrt(r2), minlength=len(q))
    print("interpolation errors", err_phi, err_g, err_G, "largest tolerance", (tol2 + tol3).max())
    assert (tol2 + tol3).max() < 1e-4 * np.abs(ref["want"][:, :3]).max()  # (the tolerance is far below the forces it is for)
    for i in range(4):
        for c in range(3):
            en = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                en.append(sw_energy(p, box6, mask, (u, gf), r_max, r_max, lam, c0, lj_pairs(p, box6, mask, r_max)))
            fd = -(en[0] - en[1]) / (2 * h)
            tol = 1.05 * (tol2[i] + tol3[i]) + 1e-8 * ref["S"][i, c]
            assert abs(fd - ref["want"][i, c]) <= tol, (i, c, fd, ref["want"][i, c], tol)
    assert np.abs(ref["want"][:, :3].sum(axis=0)).max() <= 1e-12 * ref["S"][:, :3].sum()  # Newton's third law
    assert abs(ref["ww"][6] - ref["want"][:, 3].sum()) <= 1e-12 * ref["SW"][6]
    assert abs(ref["ww"][6] - sw_energy(q, box6, mask, (u, gf), r_max, r_max, lam, c0, pairs)) < 1e-4


def test_a_silicon_crystal():
    """A perfect diamond crystal of 4 x 4 x 4 cells, 512 atoms, with silicon(): the bond angle is the tetrahedral one, so the
    three-body energy vanishes, and the bond length 2^(1/6) sigma sits in the pair minimum -epsilon: E / N = -2 epsilon within
    the interpolation error -- the property the potential was constructed to have."""
    si = sw.silicon()
    eps, sig = si["epsilon"], si["sigma"]
    bond = 2.0 ** (1.0 / 6.0) * sig
    a0 = 4.0 * bond / np.sqrt(3.0)
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]) / 4.0
    cells = np.stack(np.meshgrid(*(np.arange(4),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) + 0.125) * a0
    n = len(q)
    r_min, r_max, nk = 1.5, si["a"] * sig, 2048
    u, du = sw.pair(si["A"], si["B"], si["p"], si["q"], eps, sig, si["a"])
    gf, dgf = sw.radial(si["gamma"], sig, si["a"])
    F, U = pair_table.sample(u, du, r_min, r_max, nk)
    g, G = sw.sample(gf, dgf, r_min, r_max, nk)
    tab = SwTables(F, U, r_min, r_max, g, G, r_min, r_max, *sw.angular(si["lam"], eps, si["cos0"]))
    box6 = (4 * a0,) * 3 + (0.0, 0.0, 0.0)
    ref = sw_reference(q, box6, 7, tab, lj_pairs(q, box6, 7, r_max))
    assert n == 512 and np.all(ref["near"] == 4) and ref["triples"] == 6 * n
    x = np.linspace(2.0 ** 2, r_max ** 2, 200001)[:-1]
    err_u = np.abs(pair_table.interpolate(F, U, r_min, r_max, x)[1] - u(np.sqrt(x))).max()
    print("E/N", ref["ww"][6] / n, "three-body", ref["three"][:, 3].sum(), "err_u", err_u)
    assert abs(u(np.array([bond]))[0] + eps) < 1e-9 * eps  # the 1985 A and B put the minimum -epsilon at 2^(1/6) sigma
    assert abs(ref["three"][:, 3].sum()) < 1e-20 * n and np.abs(ref["three"][:, :3]).max() < 1e-12
    assert abs(ref["ww"][6] / n + 2.0 * eps) <= 2.0 * err_u + 1e-9 * eps and err_u < 1e-4
    assert np.abs(ref["want"][:, :3]).max() < 1e-3  # (the minimum of the interpolant sits within the interpolation error of the bond)


def test_emulation_gives_c():
    """SW_C and SW_CW = 4 x the largest |emulated - want| / (u S) of the numpy emulation (never the kernel) against the float64
    reference."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    for box, drift, kind in EMULATED:
        box6, mask = LJ_BOXES[box]
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        q = _input(box, drift)
        rng = np.random.default_rng(300)
        for T in DTYPES:  # (every constant covers both position types: in fp64 u S is only a few ulp of a result)
            f, w = sw_emulate(q, box6, mask, tab, T, rng, ref["entries"], types=types)
            r = lj_ratio(f, ref["want"], ref["S"], T).max(axis=0)
            assert w[7] == ref["ww"][7]
            rw = virial_ratio(w, ref["ww"], ref["SW"], T)
            print(box, drift, kind, np.dtype(T).name, r.round(3), rw.round(3))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, rw)
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX <= SW_C / 4
    assert worst_w.max() <= EMULATED_MAX_W <= SW_CW / 4


def test_wrong_results_are_rejected():
    """The checks under the fp32 bound (the totals under the fp64 bound) pass the float64 emulation of the rule and refuse each
    of DEFECTS: a dropped triple (the one of median |h|), G_b where G_a belongs, the slot (t_j, t_i) for (t_i, t_j), Lambda of a
    permuted triple, the third of h left out of an end, the angular term's -cs a ir_a^2 part left out, a triple counted twice
    in U (the totals alone)."""
    box, drift = "xyz", False
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    for kind in KINDS:
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        rng = np.random.default_rng(5)
        f, w = sw_emulate(q, box6, mask, tab, np.float64, rng, ref["entries"], types=types)
        check_lj(f, ref["want"], ref["S"], np.float32, c=SW_C)
        check_virial(w, ref["ww"], ref["SW"], np.float64, c=SW_CW)
        if kind == "one":
            continue  # (the typed defects need three types; the others are refused there as well)
        for defect in DEFECTS:
            f, w = sw_emulate(q, box6, mask, tab, np.float64, rng, ref["entries"], types=types, defect=defect)
            if defect == "a triple twice in U":
                check_lj(f, ref["want"], ref["S"], np.float32, c=SW_C)
            else:
                with pytest.raises(AssertionError):
                    check_lj(f, ref["want"], ref["S"], np.float32, c=SW_C)
            if defect != "no third of h for an end":  # (the totals take U from e_j itself)
                with pytest.raises(AssertionError):
                    check_virial(w, ref["ww"], ref["SW"], np.float64, c=SW_CW, count=False)
            print(kind, defect, "refused")


# ---- the 64-partner edge: built by hand on the lattice
@functools.lru_cache(maxsize=None)
def _edge(count):
    """(q, types, rc_ab, centre, reference) of an input with one centre that has exactly `count` partners within R_MAX: the xyz
    lattice, every particle of type 2 but the centre c (type 1) and k donors taken from far away (type 0) and put on the
    interstitial sites c + (+-1/2, +-1/2, +-1/2) a, c + (+-3/2, +-1/2, +-1/2) a, ... around c.  The type table leaves the pair
    (0, 2) out of the list, so the donors see c and each other and nobody else's count grows."""
    box = "xyz"
    box6, mask = LJ_BOXES[box]
    q = _input(box, False).copy()
    c = int(np.ravel_multi_index((7, 7, 7), (LJ_M,) * 3))
    base = lj_pairs(q, box6, mask, R_MAX, rows=[c])
    k = count - len(base[0])
    sites = np.array([[x, y, z] for x in (-1.5, -0.5, 0.5, 1.5) for y in (-1.5, -0.5, 0.5, 1.5) for z in (-1.5, -0.5, 0.5, 1.5)])
    sites = sites[np.argsort((sites ** 2).sum(axis=1), kind="stable")][:32]  # 8 at 0.97, 24 at 1.87
    assert 0 < k <= 32
    donors = np.arange(k)  # the first sites of the lattice: the corner of the box, far from c
    types = np.full(N, 2, dtype=np.int32)
    types[c], types[donors] = 1, 0
    q[donors, :3] = (q[c, :3] + sites[:k] * LJ_A).astype(np.float32)
    tab, _, rc_ab = _tabs("three")
    pairs = lj_pairs(q, box6, mask, R_MAX * (1 + 2.0 ** -16))
    r2 = (pairs[2] ** 2).sum(axis=1)
    listed = rc_ab(3.4)[types[pairs[0]], types[pairs[1]]] > 0
    for cut in (R_MIN, R_MAX):
        assert not np.any(np.abs(r2[listed] / cut ** 2 - 1.0) < 2.0 ** -17)
    assert r2[listed].min() > R_MIN ** 2
    ref = sw_reference(q, box6, mask, tab, pairs, types=types, rc_ab=rc_ab(3.4))
    q.setflags(write=False)
    return q, types, rc_ab, c, ref


def test_the_edge_inputs():
    """64 partners: everything finite; 65: the centre, its 65 partners and the totals NaN, everybody else finite -- more than half
    of the particles."""
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
    nl.set_sw(tab.g, tab.G, tab.r_min_3, tab.r_max_3, tab.lam, tab.cos0)


def _set(nl, kind, rc, **kw):
    """The type table (three types, at the list's cut-off), the pair table and the three-body tables onto an initialised handle."""
    tab, types, rc_ab = _tabs(kind, **kw)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    _set_tab(nl, tab)
    return tab


def _built(q, box, dtype, rc, kind, off=0, stride=4, exclusions=None, types=None, **kw):
    """(handle, device positions) after one full-list build, the tables set.  types: another type table than the kind's."""
    torch = _torch()
    nl = _handle(box, dtype, True, rc, off)
    nl.Initialize(len(q))
    _set(nl, kind, rc, **kw)
    if types is not None:
        nl.set_type_cutoffs(types, _tabs(kind)[2](rc))
    if exclusions is not None:
        nl.set_exclusions(exclusions, len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


def _lds_expected(tab, dtype):
    size = np.dtype(dtype).itemsize
    return (tab.g.size + tab.F.size) * 4 * size + 4 * 64 * (3 * size + 4) <= 65280


def _check(f, w, ref, dtype, rows=None):
    """Forces, pe_i and the totals within their bounds; returns them on the host."""
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, ref["want"], ref["S"], dtype)[slice(None) if rows is None else rows].max(axis=0).round(2),
          virial_ratio(w, ref["ww"], ref["SW"], dtype).round(2))
    check_lj(f, ref["want"], ref["S"], dtype, c=SW_C, rows=rows)
    if rows is None:
        check_virial(w, ref["ww"], ref["SW"], dtype, c=SW_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (SW_C + SW_CW) * lj_unit(dtype) * ref["SW"][6]
    return f, w


SW = contract.Consumer(
    forces="sw_forces", virial="sw_virial", scratch="sw_virial", clear="clear_sw", info="sw",
    entry=("nl_sw_forces", "nl_sw_forces_enqueue", "nl_sw_virial", "nl_sw_virial_enqueue"), set=_set, kinds=KINDS, ref=_ref,
    moved_ref=_moved_ref, extra=lambda nl: (), check=lambda f, w, x, ref, dtype, rows=None: _check(f, w, ref, dtype, rows),
    half_lists=False, local_slabs=False)
_run = functools.partial(contract.run, SW)


def _assert_nan_pattern(f, w, ref, dtype):
    """NaN exactly where the reference has it; everybody else within the bound; all 8 totals NaN."""
    f, w = f.cpu().numpy(), w.cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,) and np.isnan(ref["ww"]).all()
    assert np.array_equal(np.isnan(f), np.isnan(ref["want"]))
    clean = ~np.isnan(ref["want"]).any(axis=1)
    assert clean.sum() > len(f) // 2
    check_lj(f, ref["want"], ref["S"], dtype, c=SW_C, rows=clean)


gpu = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, dtype):
    """Every box, mask and position state x one type and three x dtype; the list cut-off, the offset width and q_stride rotate
    through the cases."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, kind in enumerate(KINDS):
        k = case + p
        rc, off, stride = (2.5, 3.4)[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        nl, qd = _built(q, box, dtype, rc, kind, off, stride)
        tab = _tabs(kind)[0]
        assert nl.sw() == dict(ntypes=tab.nt, nknots=NK, r_min=R_MIN, r_max=R_MAX, lds=_lds_expected(tab, dtype))
        assert nl.sw()["lds"] == (kind == "one" and dtype == np.float32)
        _run(nl, qd, _ref(box, drift, kind), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["three-body short", "pair short", "three-body shortest"])
def test_second_ranges(which, dtype):
    """r_max_3 != r_max, both ways, one type and three: n_in is exactly the pairs within the longer range."""
    box, drift = "tilt", True
    kw = {"three-body short": dict(r_max_3=R_22), "pair short": dict(r_max_pair=R_22), "three-body shortest": dict(r_max_3=R_18)}[which]
    for kind in KINDS:
        ref = _refs(_input(box, drift), box, kind, _pairs(box, drift), **kw)
        assert ref["ww"][7] == _ref(box, drift, kind)["ww"][7] and np.isfinite(ref["want"]).all()
        assert (ref["near"].max() < 35) == ("three-body" in which)
        nl, qd = _built(_input(box, drift), box, dtype, 2.5, kind, **kw)
        _run(nl, qd, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype,lds", [(np.float32, True), (np.float64, False)])
def test_reproducible_totals_and_both_paths(dtype, lds, monkeypatch):
    """sw_virial twice: the same bytes.  LDS against global memory on one list: the totals bit for bit, the forces (atomics) within
    the bound.  fp32 at 1024 + 1024 knots is staged (32 KiB and the strips), fp64 takes the global path by size; NL_TABLE_LDS=0
    around set_sw switches the staged one."""
    box, drift, kind = "tilt", True, "one"
    q, ref = _input(box, drift), _ref(box, drift, kind)
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nl, qd = _built(q, box, dtype, 3.4, kind)
    assert nl.sw()["lds"] == lds
    fa, wa = _run(nl, qd, ref, dtype)
    assert nl.sw_virial(qd).cpu().numpy().tobytes() == wa.tobytes() and len(wa.tobytes()) == 64
    monkeypatch.setenv("NL_TABLE_LDS", "0")
    tab = _tabs(kind)[0]
    nl.set_sw(tab.g, tab.G, tab.r_min_3, tab.r_max_3, tab.lam, tab.cos0)  # (the same tables, the same list)
    assert not nl.sw()["lds"]
    fb, wb = _run(nl, qd, ref, dtype)
    assert wa.tobytes() == wb.tobytes()
    assert np.all(np.abs(fa.astype(np.float64) - fb) <= 2 * SW_C * lj_unit(dtype) * ref["S"])


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_lambda_is_the_pair_table(kind, dtype):
    """Lambda = 0: on one full list sw_forces is table_forces byte for byte, pe_i included, and the totals are table_virial's."""
    box, drift = "xyz", True
    nl, qd = _built(_input(box, drift), box, dtype, 3.4, kind, three=False)
    f, w = nl.sw_forces(qd).cpu().numpy(), nl.sw_virial(qd).cpu().numpy()
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert np.isfinite(f).all() and np.abs(f).max() > 0.1
    assert f.tobytes() == ft.tobytes() and w.tobytes() == wt.tobytes()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_pair_table(dtype):
    box, drift, kind = "tilt", False, "three"
    q = _input(box, drift)
    ref = _refs(q, box, kind, _pairs(box, drift), pair=False)
    assert np.array_equal(ref["want"], ref["three"]) and np.abs(ref["want"][:, :3]).max() > 1 and ref["ww"][7] > N
    nl, qd = _built(q, box, dtype, 3.4, kind, pair=False)
    _run(nl, qd, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [64, 65])
def test_the_64_partner_edge(count, dtype):
    """A centre with exactly 64 partners in range is finite and within the bound; with 65, the centre, its 65 partners and all 8
    totals are NaN, every other particle is within the bound and the NaN pattern is the reference's."""
    q, types, rc_ab, c, ref = _edge(count)
    nl, qd = _built(q, "xyz", dtype, 2.5, "three", types=types)
    f, w = nl.sw_forces(qd), nl.sw_virial(qd)
    if count == 64:
        assert np.isfinite(f[c].cpu().numpy()).all()
        _check(f, w, ref, dtype)
    else:
        assert np.isnan(f[c].cpu().numpy()).all()
        _assert_nan_pattern(f, w, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_partner_below_the_radial_table(dtype):
    """One particle moved to 0.5 from its neighbour: below r_min_3 = 0.85, inside the pair table (sampled from 0.4 here).  Both are
    centres with a partner below the table: NaN for them and all their partners in range, and in all 8 totals."""
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
    _assert_nan_pattern(nl.sw_forces(qd), nl.sw_virial(qd), ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_exclusions(dtype):
    """A list filtered by nl_set_exclusions (the bonds along x): an excluded partner forms no pair term and no triple; the
    unfiltered reference is refused."""
    box, kind = "xyz", "one"
    q = _input(box, False)
    ref = _refs(q, box, kind, _pairs(box, False), exclusions=_bonds())
    assert ref["near"].max() <= 47 and ref["ww"][7] == _ref(box, False, kind)["ww"][7] - N
    nl, qd = _built(q, box, dtype, 2.5, kind, exclusions=_bonds())
    f, _ = _run(nl, qd, ref, dtype)
    with pytest.raises(AssertionError):
        check_lj(f, _ref(box, False, kind)["want"], ref["S"], dtype, c=SW_C)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,kind", [("xyz", "one"), ("tilt", "three")])
def test_reuse_within_the_skin(box, kind, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants; no extra build."""
    contract.reuse_within_the_skin(SW, box, kind, True, dtype)


@gpu
def test_captured():
    """A capture of sw_virial before its first call is NL_ERR_STATE (the scratch cannot be allocated); after one synchronous call
    one graph holds the copy of the positions, the update, the forces and the totals, replayed at two position sets."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()

    def before(nl, qd, fd, wd):
        nl.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0):
            with pytest.raises(NLError) as e:
                nl.sw_virial(qd, wait=False, out=wd)
            assert e.value.code == NL_ERR_STATE
            nl.sw_forces(qd, wait=False, out=fd)  # (the forces need no scratch)
        nl.sw_virial(qd)  # synchronous, outside a capture: allocates

    contract.captured(SW, True, before, lambda nl, replay: None)  # (nothing is set afterwards)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces and totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat all are finite."""
    def set_tables(nl):
        nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, R_MAX, NK), 1e-3, R_MAX)  # (a uniform random box has close pairs)
        gs, dgs = sw_functions(1)
        nl.set_sw(*sw.sample(gs[0][0], dgs[0][0], 1e-3, 1.5, NK), 1e-3, 1.5, *sw_angular(1))  # (about 13 partners within 1.5)

    def prepare(nl, qd):
        nl.update(qd, sync=True)
        nl.sw_virial(qd)  # (the scratch)

    contract.failed_list(SW, set_tables, prepare)


@gpu
@pytest.mark.parametrize("off", [32, 64])
def test_both_offset_widths(off):
    contract.both_offset_widths(SW, True, off)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    tab, _, _ = _tabs("one")
    tab3, types, rc_ab = _tabs("three")
    F, U = tab.F[0], tab.U[0]
    q = _input("open", False)
    nl = _handle("open", np.float32, True, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    calls = contract.entry_calls(SW, lib, fd, out)
    set_one = lambda t=tab: nl.set_sw(t.g, t.G, t.r_min_3, t.r_max_3, t.lam, t.cos0)  # noqa: E731
    # nothing set; only the pair table; only the g tables
    assert nl.sw() is None and lib.nl_get_sw(nl._h, *([None] * 5)) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for have_pair, have_sw in ((False, False), (True, False), (False, True)):
        nl.set_pair_table(F, U, R_MIN, R_MAX) if have_pair else nl.clear_pair_table()
        set_one() if have_sw else nl.clear_sw()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    want = nl.sw_virial(qd).cpu().numpy()
    assert np.isfinite(want).all()
    # the setter's arguments: each refused, and the tables that were set are kept
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    g, G = tab.g[0].copy(), tab.G[0].copy()
    bad_g, bad_G = g.copy(), G.copy()
    bad_g[5], bad_G[7] = np.inf, np.nan
    big = np.zeros(4097)
    good = dict(nt=1, nk=NK, lo=R_MIN, hi=R_MAX, g=g, G=G, lam=np.array([2.0]), c0=np.array([-1 / 3]))
    keep = []  # (the arrays behind the pointers)

    def args(**kw):
        a = dict(good, **kw)
        ptrs = {k: None if a[k] is None else dp(a[k]) for k in ("g", "G", "lam", "c0")}
        keep.append(ptrs)
        return a["nt"], a["nk"], a["lo"], a["hi"], ptrs["g"], ptrs["G"], ptrs["lam"], ptrs["c0"]

    lam3, c03 = tab3.lam.copy(), tab3.cos0.copy()
    lam3[1, 0, 2] += 0.5  # not symmetric in the ends
    c03[2, 1, 0] = -c03[2, 0, 1]
    for kw in (dict(g=None), dict(G=None), dict(lam=None), dict(c0=None), dict(nk=1), dict(nk=-2), dict(nk=4097, g=big, G=big), dict(lo=0.0),
               dict(lo=-1.0), dict(lo=R_MAX), dict(hi=np.inf), dict(lo=np.nan), dict(nt=0), dict(nt=5), dict(g=bad_g), dict(G=bad_G),
               dict(lam=np.array([np.inf])), dict(lam=np.array([np.nan])), dict(c0=np.array([1.0 + 1e-12])), dict(c0=np.array([-1.5])),
               dict(c0=np.array([np.nan])), dict(nt=3, g=tab3.g, G=tab3.G, lam=lam3, c0=tab3.cos0),
               dict(nt=3, g=tab3.g, G=tab3.G, lam=tab3.lam, c0=c03)):
        assert lib.nl_set_sw(nl._h, *args(**kw)) == NL_ERR_ARG, kw.keys()
        assert nl.sw()["nknots"] == NK and nl.sw()["ntypes"] == 1
    assert lib.nl_set_sw(None, *args()) == NL_ERR_ARG
    assert lib.nl_set_sw(nl._h, *args(c0=np.array([1.0]))) == 0 and lib.nl_set_sw(nl._h, *args(c0=np.array([-1.0]))) == 0
    set_one()
    assert nl.sw_virial(qd).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(TypeError):
        nl.set_sw(g, G[:-1], R_MIN, R_MAX, 2.0, -0.3)
    with pytest.raises(TypeError):
        nl.set_sw(tab3.g, tab3.G, R_MIN, R_MAX, 2.0, -0.3)  # 9 slots, one triple
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_one)
    # reach of the g tables (the pair table stays at 2.5); from 2.7 on some centres have more than 64 partners in range
    gs, dgs = sw_functions(1)
    contract.reach(SW, nl, qd, lambda r_max: nl.set_sw(*sw.sample(gs[0][0], dgs[0][0], R_MIN, r_max, NK), R_MIN, r_max, 2.0, -0.3))
    # ... and of the pair table
    set_one()
    nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, 2.7, NK), R_MIN, 2.7)
    nl.sw_forces(qd)
    with pytest.raises(NLError) as e:
        nl.sw_forces(qd, wait=False)
    assert e.value.code == NL_ERR_ARG
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    contract.clearing(SW, nl, qd, set_one, lambda: lib.nl_set_sw(nl._h, *args(nk=0)))
    # several types: a type table of that ntypes, a pair table of 1 or ntypes types
    contract.several_types(SW, nl, qd, types, set_one, lambda: set_one(tab3))  # (a pair table of one type under nine g slots)
    nl.set_pair_table(tab3.F, tab3.U, R_MIN, R_MAX)
    assert torch.isfinite(nl.sw_forces(qd)).all()
    # a half list
    half = _handle("open", np.float32, False, 2.9)
    half.Initialize(N)
    _set_tab(half, tab)
    half.MakeNeighList(qd, N)
    assert torch.isfinite(half.table_forces(qd)).all()  # (the pair table's calls take this list)
    for fn, o in calls:
        assert fn(half._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    contract.no_particles(SW, lib, True, lambda empty: _set_tab(empty, tab), qd, fd, out)


@gpu
def test_slab_lists_are_refused():
    """A full-list slab build, with and without nl_set_local_ids: NL_ERR_STATE from all four calls (the force on an owned end needs
    the triples centred on ghosts)."""
    contract.slab_lists_are_refused(SW, True)


@gpu
def test_distributed_lists_are_refused():
    """A distributed build of a world of one (nl_make_list_distributed: the whole box, the global ids in w): its list holds
    caller ids, and all four calls are NL_ERR_STATE, wait and enqueue."""
    contract.distributed_lists_are_refused(SW, True)

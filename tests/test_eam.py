"""Embedded-atom potentials (nl_set_eam, nl_eam_forces, nl_eam_virial, their enqueue variants, nl_eam_get_density) against an
O(N^2) float64 evaluation of the rule, with an error bound per particle and per component.

Contract tested (include/nl_hip.h, nl_set_eam):
  * |rho - want| <= EAM_C_RHO u S_rho, S_rho the uncancelled sum of the density reads (|f_k| + |f_k+1| + |df_k| r2 / D);
  * |got - want| <= EAM_C u S for every particle and each of fx, fy, fz, pe on its own, and <= EAM_CW u S for each of the 7 sums
    of the totals, n_in exact.  want: tests.util_eam eam_reference (eam.density, eam.embed and pair_table.interpolate on the
    caller's double tables, no list).  S: per pair (m_phi + MP_i mG_j + MP_j mG_i) |d_c|, where m_phi, mG are the three terms of
    a table read (section 8o) and MP_i = |P_k| + |P_k+1| + |dP_k| (rho_i + S_rho_i) / Drho is the read of F' with its
    conditioning on rho's own error, for both ends of the pair; pe_i has half the pair energies' magnitudes plus ME_i, the
    same expression on E;
  * NaN rules, LDS against global, half against full, the enqueue variants, state and arguments.

The constants are not fitted to the kernel.  Each is 4 x the largest ratio that a numpy emulation of the three passes in the
position type reaches against the float64 reference (tests.util_eam eam_emulate: one rounding per operation, no FMA, random
summation order, knots and scalars rounded as the setters round them; the totals with the kernels' summation tree) over the
inputs of EMULATED, in float32 and in float64: 1.82 per particle and column (the energies, either type; the force components
reach 0.49: EAM_C = 7.28), 2.35 for rho (float64; float32 1.76: EAM_C_RHO = 9.4), 0.391 for the totals (U in float64; the virial
0.116: EAM_CW = 1.57).  test_emulation_gives_c recomputes them.  The
factor 4 covers the GPU's other summation order within a row.

The inputs are those of tests/test_pair_table.py: the 14^3 jittered lattice, n = 2744 > 4 NL_TABLE_BLOCKS rows, no pair within
2^-17 (relative, r^2) of r_max or r_min; the density tables use the pair table's grid (R_MIN, R_MAX), so the band check covers
both; test_unequal_ranges and test_a_density_beyond_rho_max also put one of the two ranges at R_SHORT = 2.2, off whose band
the inputs lie as well (test_unequal_ranges_are_told_apart).  The potential (tests.util_eam eam_functions): f_b = A_b exp(-beta_b (r - r_e)), F_a = -C_a sqrt(rho + 1) + D_a rho^2,
phi the Morse potentials of test_pair_table; none vanishes at r_max, so a dropped pair is visible.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import eam, pair_table
from tests import consumer_contract as contract
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _handle, _pair_tab, _tab, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_unit
from tests.util_eam import (DEFECTS, EAM_C, EAM_C_RHO, EAM_CW, EamTables, eam_emulate, eam_energy, eam_functions, eam_list_pairs,
                            eam_reference)
from tests.util_table import morse
from tests.virial_util import check_virial, virial_ratio

NBLK = 512  # NL_TABLE_BLOCKS of include/nl_hip.h
KINDS = ("one", "three")
R_SHORT = 2.2  # a second range, for tables whose r_max differ (test_unequal_ranges*)
RHO_MAX = {"one": 22.5, "three": 27.5}  # about 1.5 x the largest density of any input (test_inputs)
EMULATED = [("open", False, "one"), ("xyz", False, "one"), ("tilt", True, "one"), ("xyz", True, "three"), ("tilt", False, "three"),
            ("open", False, "three")]
EMULATED_MAX, EMULATED_MAX_RHO, EMULATED_MAX_W = 1.82, 2.35, 0.391  # the largest ratios of test_emulation_gives_c


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _tabs(kind, nk=NK, nke=NK, embedding=True, pair=True, rho_max=None, r_min_pair=R_MIN, r_max_pair=R_MAX, r_max_d=R_MAX):
    """(EamTables, types, rc_ab(rc_list)) of a potential: one type with the Morse table, or the 3-type mixture of
    lj_type_params(3, 3.4) with the typed Morse table, whose pair (0, 2) the type table leaves out of the list.  The pair table
    lies on (r_min_pair, r_max_pair), the density tables on (R_MIN, r_max_d)."""
    nt = 1 if kind == "one" else 3
    F, U, types, rc_ab = _tab("morse" if nt == 1 else "typed3", nk)
    if (r_min_pair, r_max_pair) != (R_MIN, R_MAX):
        F, U = _pair_tab(nt, r_min_pair, r_max_pair, nk)
    fs, dfs, Fs, dFs = eam_functions(nt)
    rho_max = RHO_MAX[kind] if rho_max is None else rho_max
    f, G, E, P = eam.sample(fs, dfs, Fs, dFs, R_MIN, r_max_d, nk, rho_max, nke)
    if not embedding:
        E, P = np.zeros_like(E), np.zeros_like(P)
    if not pair:
        F, U = np.zeros_like(F), np.zeros_like(U)
    return EamTables(F, U, r_min_pair, r_max_pair, f, G, R_MIN, r_max_d, E, P, rho_max), types, rc_ab


def _refs(q, box, kind, pairs, **kw):
    box6, mask = LJ_BOXES[box]
    tab, types, rc_ab = _tabs(kind, **kw)
    return eam_reference(q, box6, mask, tab, pairs=pairs, types=types, rc_ab=None if rc_ab is None else rc_ab(3.4))


@functools.lru_cache(maxsize=None)
def _ref(box, drift, kind):
    return _refs(_input(box, drift), box, kind, _pairs(box, drift))


@functools.lru_cache(maxsize=None)
def _moved_ref(box, kind, seed=21):
    q, pairs = _moved(box, seed)
    return _refs(q, box, kind, pairs)


def _list_pairs(box, drift, kind):
    """(I, J) of the ordered pairs a full list holds: the type table's pair (0, 2) left out."""
    tab, types, rc_ab = _tabs(kind)
    return eam_list_pairs(tab, _pairs(box, drift), types, None if rc_ab is None else rc_ab(3.4))[:2]


def _weakest(kind):
    """What a single pair at r_max gives at least: (|F_phi(r_max)| r_max, |U(r_max)| / 2, f(r_max)) of the weakest live slot.
    The embedding term has the sign of the pair term there (test_inputs), so it only adds."""
    tab = _tabs(kind)[0]
    live = np.abs(tab.F).sum(axis=1) > 0
    return (np.abs(tab.F[live, -1]) * R_MAX).min(), (0.5 * np.abs(tab.U[live, -1])).min(), tab.f[:, -1].min()


def _rho_ratio(rho, ref, dtype):
    return np.abs(np.asarray(rho, dtype=np.float64) - ref["rho"]) / (lj_unit(dtype) * ref["S_rho"])


# ------------------------------------------------------------------------------------------------- CPU: the checker
def test_header_states_the_constants():
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    assert int(re.search(r"#define NL_TABLE_BLOCKS\s+(\d+)", text).group(1)) == NBLK
    assert int(re.search(r"#define NL_TABLE_MAX_KNOTS\s+(\d+)", text).group(1)) == 4096
    assert int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1)) == 65280
    assert int(re.search(r"#define NL_MAX_TYPES\s+(\d+)", text).group(1)) == 32
    assert N == 2744 > 4 * NBLK  # some waves of the persistent grid walk a second row
    for name in ("nl_set_eam", "nl_get_eam", "nl_eam_forces", "nl_eam_forces_enqueue", "nl_eam_virial", "nl_eam_virial_enqueue",
                 "nl_eam_get_density"):
        assert re.search(r"\bint %s\(" % name, text), name


def test_inputs():
    """Every reference density lies in (0, rho_max), rho_max is about 1.5 x the largest; the potential does not vanish at r_max
    and its embedding term pulls the way its pair term does there."""
    for kind in KINDS:
        top = 0.0
        for box, drift in CASES:
            ref = _ref(box, drift, kind)
            assert np.all((ref["rho"] > 0) & (ref["rho"] < RHO_MAX[kind]))
            assert np.isfinite(ref["want"]).all() and np.isfinite(ref["ww"]).all() and np.all(ref["fp"] < 0)
            top = max(top, ref["rho"].max())
        for box in ("xyz", "tilt"):
            top = max(top, _moved_ref(box, kind)["rho"].max())
            assert _moved_ref(box, kind)["rho"].max() < RHO_MAX[kind]
        print(kind, "largest rho", top)
        assert 1.4 * top <= RHO_MAX[kind] <= 1.6 * top
        tab = _tabs(kind)[0]
        assert np.all(tab.G[:, -1] > 0) and np.all(tab.F[:, -1] <= 0) and np.all(tab.U[:, -1] <= 0)
        Fm, Um, fm = _weakest(kind)
        assert Fm > 0.03 and Um > 0.008 and fm > 0.03
    tab, types, rc_ab = _tabs("three")
    assert tab.f.shape == (3, NK) and tab.E.shape == (3, NK) and tab.F.shape == (6, NK) and rc_ab(3.4)[0, 2] == 0


def test_the_rule_in_float64():
    """eam.density and eam.embed are the stated rule, and eam_reference is the plain double loop over all pairs."""
    E, P = np.array([1.0, 3.0, 2.0]), np.array([0.5, 0.25, -1.0])
    Fe, fp = eam.embed(E, P, 4.0, np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.0 + 1e-12, -1e-12, np.nan]))
    assert np.array_equal(Fe[:5], [1.0, 2.0, 3.0, 2.5, 2.0]) and np.array_equal(fp[:5], [0.5, 0.375, 0.25, -0.375, -1.0])
    assert np.isnan(Fe[5:]).all() and np.isnan(fp[5:]).all()
    f, G = np.array([4.0, 2.0, 1.0]), np.array([8.0, 0.0, -4.0])
    fv, Gv, inn = eam.density(f, G, 1.0, 3.0, np.array([1.0, 3.0, 5.0, 8.999, 9.0, 0.5, 0.0]))  # knots at r^2 = 1, 5, 9
    assert np.array_equal(fv[:3], [4.0, 3.0, 2.0]) and np.array_equal(Gv[:3], [8.0, 4.0, 0.0]) and abs(fv[3] - 1.0) < 1e-3
    assert fv[4] == 0 and Gv[4] == 0 and np.isnan(fv[5]) and np.isnan(Gv[5]) and fv[6] == 0
    assert np.array_equal(inn, [True, True, True, True, False, True, False])
    fs, dfs, Fs, dFs = eam_functions(2)
    f2, G2, E2, P2 = eam.sample(fs, dfs, Fs, dFs, 0.5, 1.8, 64, 30.0, 32)
    r = pair_table.knots(0.5, 1.8, 64)
    assert f2.shape == (2, 64) and np.allclose(f2[1], fs[1](r)) and np.allclose(G2[0], -dfs[0](r) / r)
    assert np.allclose(E2[1], Fs[1](eam.rho_knots(30.0, 32))) and np.allclose(P2[0], dFs[0](eam.rho_knots(30.0, 32)))
    f1 = eam.sample(fs[0], dfs[0], Fs[0], dFs[0], 0.5, 1.8, 64, 30.0, 32)
    assert f1[0].shape == (64,) and np.array_equal(f1[0], f2[0]) and np.array_equal(f1[3], P2[0])
    # the double loop, open box, two types
    rng = np.random.default_rng(2)
    g = np.stack(np.meshgrid(*(np.arange(3),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = g * 1.1 + rng.uniform(-0.1, 0.1, size=g.shape)
    types = rng.integers(0, 2, size=len(q))
    F, U = pair_table.sample(*morse(), 0.5, 1.8, 64)
    tab = EamTables(F, U, 0.5, 1.8, f2, G2, 0.5, 1.8, E2, P2, 30.0)
    ref = eam_reference(q, (9.0, 9.0, 9.0, 0.0, 0.0, 0.0), 0, tab, types=types)
    n = len(q)
    rho = np.zeros(n)
    for i in range(n):
        for j in range(n):
            r2 = ((q[i] - q[j]) ** 2).sum()
            if i != j and r2 < 1.8 ** 2:
                rho[i] += eam.density(f2[types[j]], G2[types[j]], 0.5, 1.8, r2)[0]
    emb = [eam.embed(E2[types[i]], P2[types[i]], 30.0, rho[i]) for i in range(n)]
    want = np.zeros((n, 4))
    for i in range(n):
        want[i, 3] = emb[i][0]
        for j in range(n):
            d = q[i] - q[j]
            r2 = (d * d).sum()
            if i != j and r2 < 1.8 ** 2:
                fr, pe, _ = pair_table.interpolate(F, U, 0.5, 1.8, r2)
                Gi, Gj = (eam.density(f2[types[k]], G2[types[k]], 0.5, 1.8, r2)[1] for k in (i, j))
                want[i, :3] += (fr + emb[i][1] * Gj + emb[j][1] * Gi) * d
                want[i, 3] += 0.5 * pe
    assert np.allclose(ref["rho"], rho, rtol=1e-13) and np.allclose(ref["want"], want, rtol=1e-12, atol=1e-13)
    assert abs(ref["ww"][6] - want[:, 3].sum()) < 1e-11 and np.abs(ref["want"][:, :3].sum(axis=0)).max() < 1e-11


def test_sampled_tables_converge():
    """Density and embedding tables against the functions they sample, on dense grids: the largest error falls 4 x per doubling
    of the knots."""
    fs, dfs, Fs, dFs = eam_functions(3)
    x = np.linspace(0.92 ** 2, R_MAX ** 2, 100001)[:-1]
    rho = np.linspace(0.0, RHO_MAX["three"], 100001)
    worst = []
    for nk in (256, 512, 1024, 2048):
        f, G, E, P = eam.sample(fs, dfs, Fs, dFs, R_MIN, R_MAX, nk, RHO_MAX["three"], nk)
        w = []
        for b in range(3):
            fv, Gv, inn = eam.density(f[b], G[b], R_MIN, R_MAX, x)
            Fe, fp = eam.embed(E[b], P[b], RHO_MAX["three"], rho)
            r = np.sqrt(x)
            assert inn.all()
            w += [np.abs(fv - fs[b](r)).max(), np.abs(Gv + dfs[b](r) / r).max(), np.abs(Fe - Fs[b](rho)).max(), np.abs(fp - dFs[b](rho)).max()]
        worst.append(w)
    ratios = np.array(worst[:-1]) / np.array(worst[1:])
    print("largest errors per nknots", worst, "ratios", ratios)
    assert np.all((ratios > 3.0) & (ratios < 5.0))


def test_reference_is_the_gradient_of_its_energy():
    """eam_reference's forces at 4096 knots against the central difference of the ANALYTIC energy, tilted and periodic, two
    types.  The tolerance is the interpolation error of the tables, measured per table on a dense grid (it falls 4 x per
    doubling: test_sampled_tables_converge) and carried through the rule: per pair err_phi + (|fp_i| + |fp_j|) err_G +
    (|G_j| dfp_i + |G_i| dfp_j), dfp = err_P + max |F''| (partners) err_f; plus the truncation error of the difference."""
    rng = np.random.default_rng(3)
    m, a = 5, 1.125
    box6, mask = (m * a, m * a, m * a, a, -a, 2 * a), 7
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (g + 0.5) * a + rng.uniform(-0.1, 0.1, size=g.shape)
    r_min, r_max, rho_max, nk, h = 0.5, 1.8, 30.0, 4096, 1e-5
    types = rng.integers(0, 2, size=len(q))
    u, du = morse()
    fs, dfs, Fs, dFs = eam_functions(2)
    F, U = pair_table.sample(u, du, r_min, r_max, nk)
    f, G, E, P = eam.sample(fs, dfs, Fs, dFs, r_min, r_max, nk, rho_max, nk)
    tab = EamTables(F, U, r_min, r_max, f, G, r_min, r_max, E, P, rho_max)
    ref = eam_reference(q, box6, mask, tab, types=types, parts=True)
    I, J, d, _, _, _, _ = ref["pairs"]
    r = np.sqrt((d * d).sum(axis=1))
    assert np.abs(r - r_max).min() > 10 * h and ref["rho"].max() < rho_max
    x = np.linspace(0.8 ** 2, r_max ** 2, 400001)[:-1]
    rr = np.sqrt(x)
    rho = np.linspace(0.0, rho_max, 400001)
    err_phi = np.abs(pair_table.interpolate(F, U, r_min, r_max, x)[0] + du(rr) / rr).max()
    err_f = max(np.abs(eam.density(f[b], G[b], r_min, r_max, x)[0] - fs[b](rr)).max() for b in range(2))
    err_G = max(np.abs(eam.density(f[b], G[b], r_min, r_max, x)[1] + dfs[b](rr) / rr).max() for b in range(2))
    err_P = max(np.abs(eam.embed(E[b], P[b], rho_max, rho)[1] - dFs[b](rho)).max() for b in range(2))
    ke = (ref["rho"] / tab.drho).astype(np.int64)  # max |F''| on the segments around each particle's density
    F2 = np.array([np.abs(np.diff(P[t])[k - 1:k + 2]).max() for t, k in zip(types, ke)]) / tab.drho
    partners = np.bincount(I, minlength=len(q))
    dfp = err_P + F2 * partners * err_f
    Gi = np.array([eam.density(f[types[i]], G[types[i]], r_min, r_max, x2)[1] for i, x2 in zip(I, r * r)])
    Gj = np.array([eam.density(f[types[j]], G[types[j]], r_min, r_max, x2)[1] for j, x2 in zip(J, r * r)])
    per_pair = err_phi + (np.abs(ref["fp"][I]) + np.abs(ref["fp"][J])) * err_G + np.abs(Gj) * dfp[I] + np.abs(Gi) * dfp[J]
    print("interpolation errors", err_phi, err_f, err_G, err_P, "largest pair tolerance", per_pair.max())
    assert per_pair.max() < 1e-4
    for i in range(4):
        for c in range(3):
            e = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                e.append(eam_energy(p, box6, mask, (u, fs, Fs), r_max, types))
            fd = -(e[0] - e[1]) / (2 * h)
            tol = 1.05 * (per_pair * np.abs(d[:, c]))[I == i].sum() + 1e-8 * ref["S"][i, c]  # (h^2 f''' / 6 and the difference's rounding)
            assert abs(fd - ref["want"][i, c]) <= tol, (i, c, fd, ref["want"][i, c], tol)
    assert np.abs(ref["want"][:, :3].sum(axis=0)).max() <= 1e-12 * ref["S"][:, :3].sum()  # Newton's third law
    assert abs(ref["ww"][6] - ref["want"][:, 3].sum()) <= 1e-12 * ref["SW"][6]
    assert abs(ref["ww"][6] - eam_energy(q, box6, mask, (u, fs, Fs), r_max, types)) < 1e-4


def test_emulation_gives_c():
    """EAM_C, EAM_C_RHO and EAM_CW = 4 x the largest |emulated - want| / (u S) of the numpy emulation (never the kernel)
    against the float64 reference."""
    worst, worst_rho, worst_w = np.zeros(4), 0.0, np.zeros(7)
    for box, drift, kind in EMULATED:
        box6, mask = LJ_BOXES[box]
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        pairs = _list_pairs(box, drift, kind)
        q = _input(box, drift)
        for order in range(2):
            rng = np.random.default_rng(200 + order)
            for T in DTYPES:  # (every constant covers both position types: in fp64 u S is only a few ulp of a result)
                f, rho, w = eam_emulate(q, box6, mask, tab, T, rng, pairs, types=types)
                r = lj_ratio(f, ref["want"], ref["S"], T).max(axis=0)
                rr = _rho_ratio(rho, ref, T).max()
                assert w[7] == ref["ww"][7]
                rw = virial_ratio(w, ref["ww"], ref["SW"], T)
                print(box, drift, kind, order, np.dtype(T).name, r.round(2), round(float(rr), 2), rw.round(2))
                worst, worst_rho, worst_w = np.maximum(worst, r), max(worst_rho, rr), np.maximum(worst_w, rw)
    print("largest ratio per column", worst, worst_rho, worst_w)
    assert worst.max() <= EMULATED_MAX <= EAM_C / 4
    assert worst_rho <= EMULATED_MAX_RHO <= EAM_C_RHO / 4
    assert worst_w.max() <= EMULATED_MAX_W <= EAM_CW / 4


def _sharp(ref, kind):
    Fm, Um, fm = _weakest(kind)
    u = lj_unit(np.float32)
    assert np.all(EAM_C * u * ref["S"][:, :3].max(axis=1) <= 0.25 * Fm / np.sqrt(3.0)), EAM_C * u * ref["S"][:, :3].max() / Fm
    assert np.all(EAM_C * u * ref["S"][:, 3] <= 0.25 * Um), EAM_C * u * ref["S"][:, 3].max() / Um
    assert np.all(EAM_C_RHO * u * ref["S_rho"] <= 0.25 * fm), EAM_C_RHO * u * ref["S_rho"].max() / fm


def test_bound_is_sharp():
    """On every input the bounds stay below a quarter of what the weakest single pair at r_max gives a component, an energy, a
    density."""
    seen = 0
    for box, drift in CASES:
        for kind in KINDS:
            _sharp(_ref(box, drift, kind), kind)
            seen += 1
    for box in ("xyz", "tilt"):
        for kind in KINDS:
            _sharp(_moved_ref(box, kind), kind)
    assert seen == 18


def _check_arrays(f, rho, w, ref, dtype):
    check_lj(f, ref["want"], ref["S"], dtype, c=EAM_C)
    assert _rho_ratio(rho, ref, dtype).max() <= EAM_C_RHO
    check_virial(w, ref["ww"], ref["SW"], dtype, c=EAM_CW, count=False)


def test_wrong_results_are_rejected():
    """The checks under the fp32 bound (the totals under the fp64 bound) pass the float64 emulation of the rule and refuse each
    of DEFECTS: a pair dropped from the density, f of the row's type where the partner's belongs (3 types), fp_i used for both
    ends, Fe left out of pe_i, the half list's missing reaction in rho."""
    box, drift = "xyz", False
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    for kind in KINDS:
        tab, types, _ = _tabs(kind)
        ref = _ref(box, drift, kind)
        pairs = _list_pairs(box, drift, kind)
        rng = np.random.default_rng(5)
        f, rho, w = eam_emulate(q, box6, mask, tab, np.float64, rng, pairs, types=types)
        _check_arrays(f, rho, w, ref, np.float32)
        check_virial(w, ref["ww"], ref["SW"], np.float64, c=EAM_CW)
        for defect in DEFECTS:
            if defect == "f of the row's type" and kind == "one":
                continue
            f, rho, w = eam_emulate(q, box6, mask, tab, np.float64, rng, pairs, types=types, defect=defect)
            if defect == "Fe left out":
                assert _rho_ratio(rho, ref, np.float32).max() <= EAM_C_RHO
            else:
                assert _rho_ratio(rho, ref, np.float32).max() > EAM_C_RHO or defect == "fp_i for both ends", defect
            with pytest.raises(AssertionError):
                check_lj(f, ref["want"], ref["S"], np.float32, c=EAM_C)
            if defect == "fp_i for both ends" and kind == "one":
                continue  # (one density slot: G_i = G_j, and the two rows of a pair then add up to the right W and U)
            with pytest.raises(AssertionError):
                check_virial(w, ref["ww"], ref["SW"], np.float64, c=EAM_CW, count=False)
            print(kind, defect, "refused")


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _set(nl, kind, rc, **kw):
    """The type table (three types, at the list's cut-off), the pair table and the EAM tables onto an initialised handle."""
    tab, types, rc_ab = _tabs(kind, **kw)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    nl.set_pair_table(tab.F if tab.nt_pair > 1 else tab.F[0], tab.U if tab.nt_pair > 1 else tab.U[0], tab.r_min, tab.r_max)
    nl.set_eam(tab.f, tab.G, tab.r_min_d, tab.r_max_d, tab.E, tab.P, tab.rho_max)
    return tab


def _check(f, rho, w, ref, dtype, rows=None):
    """Forces and pe_i, rho and the totals within their bounds; returns them on the host."""
    f, rho, w = f.cpu().numpy(), rho.cpu().numpy(), w.cpu().numpy()
    rr = _rho_ratio(rho, ref, dtype)
    print(np.dtype(dtype).name, lj_ratio(f, ref["want"], ref["S"], dtype)[slice(None) if rows is None else rows].max(axis=0).round(2),
          rr.max().round(2), virial_ratio(w, ref["ww"], ref["SW"], dtype).round(2))
    check_lj(f, ref["want"], ref["S"], dtype, c=EAM_C, rows=rows)
    assert rr[slice(None) if rows is None else rows].max() <= EAM_C_RHO
    if rows is None:
        check_virial(w, ref["ww"], ref["SW"], dtype, c=EAM_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (EAM_C + EAM_CW) * lj_unit(dtype) * ref["SW"][6]
    return f, rho, w


EAM = contract.Consumer(
    forces="eam_forces", virial="eam_virial", scratch="eam_virial", clear="clear_eam", info="eam",
    entry=("nl_eam_forces", "nl_eam_forces_enqueue", "nl_eam_virial", "nl_eam_virial_enqueue"), set=_set, kinds=KINDS, ref=_ref,
    moved_ref=_moved_ref, extra=lambda nl: nl.eam_density(),  # (rho, fp)
    check=lambda f, w, x, ref, dtype, rows=None: _check(f, x[0], w, ref, dtype, rows), half_lists=True, local_slabs=False)
_built = functools.partial(contract.built, EAM)
_run = functools.partial(contract.run, EAM)
gpu = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x one type and three x list kind x dtype; the list cut-off, the offset width and
    q_stride rotate through the cases.  fp_i is F' of the rho_i the call returns."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, kind in enumerate(KINDS):
        k = case + p + (1 if full else 0)
        rc, off, stride = (2.5, 3.4)[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        nl, qd = _built(q, box, dtype, full, rc, kind, off, stride)
        info = nl.eam()
        tab = _tabs(kind)[0]
        knot = 4 * np.dtype(dtype).itemsize  # (three types: 6 pair slots and 3 density slots of 1024 knots do not fit together)
        assert info == dict(ntypes=tab.nt, nknots_d=NK, r_min=R_MIN, r_max=R_MAX, nknots_e=NK, rho_max=RHO_MAX[kind],
                            lds_density=tab.f.size * knot <= 65280, lds_forces=(tab.f.size + tab.F.size) * knot <= 65280)
        assert info["lds_forces"] == (kind == "one" and dtype == np.float32)
        ref = _ref(box, drift, kind)
        _run(nl, qd, ref, dtype)
        rho, fp = (v.cpu().numpy().astype(np.float64) for v in nl.eam_density())
        tab, types, _ = _tabs(kind)
        ty = np.zeros(N, dtype=np.int64) if types is None else types
        for a in range(tab.nt):
            want = eam.embed(tab.E[a], tab.P[a], tab.rho_max, rho[ty == a])[1]
            assert np.all(np.abs(fp[ty == a] - want) <= 8 * lj_unit(dtype) * (np.abs(tab.P[a]).max() + np.abs(np.diff(tab.P[a])).max() * NK))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "three"), ("xyz", False, "one")])
def test_half_and_full_agree(box, drift, kind, dtype):
    ref = _ref(box, drift, kind)
    got = {}
    for full in (False, True):
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, kind)
        got[full] = _run(nl, qd, ref, dtype)
    u = lj_unit(dtype)
    assert np.all(np.abs(got[False][0].astype(np.float64) - got[True][0]) <= 2 * EAM_C * u * ref["S"])
    assert np.all(np.abs(got[False][1].astype(np.float64) - got[True][1]) <= 2 * EAM_C_RHO * u * ref["S_rho"])
    assert np.all(np.abs(got[False][2][:7] - got[True][2][:7]) <= 2 * EAM_CW * u * ref["SW"])
    assert got[False][2][7] == got[True][2][7] == ref["ww"][7]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_full_list_is_reproducible(kind, dtype):
    """No atomics after a full build: two calls give the same bytes -- forces, rho, fp and the totals."""
    nl, qd = _built(_input("tilt", True), "tilt", dtype, True, 3.4, kind)
    runs = []
    for _ in range(2):
        f, w = nl.eam_forces(qd), nl.eam_virial(qd)
        runs.append([v.cpu().numpy().tobytes() for v in (f, w) + nl.eam_density()])
    assert runs[0] == runs[1] and len(runs[0][1]) == 64


@gpu
@pytest.mark.parametrize("dtype,nk,lds", [(np.float32, 1024, True), (np.float64, 1024, False), (np.float64, 512, True)])
def test_lds_and_global_paths(dtype, nk, lds, monkeypatch):
    """On one full list the LDS and the global path are bit for bit equal: forces, rho and the totals.  fp32 at 1024 + 1024
    knots is staged (32 KiB), fp64 at 1024 + 1024 takes the global path by size (2 x 32 KiB > NL_TABLE_LDS_BYTES; its density
    pass still stages its own 32 KiB), fp64 at 512 + 512 is staged; NL_TABLE_LDS=0 around set_eam switches all passes."""
    box, drift, kind = "tilt", True, "one"
    q = _input(box, drift)
    ref = _refs(q, box, kind, _pairs(box, drift), nk=nk)
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nl, qd = _built(q, box, dtype, True, 3.4, kind, nk=nk)
    assert nl.eam()["lds_forces"] == lds and nl.eam()["lds_density"]
    a = _run(nl, qd, ref, dtype)
    monkeypatch.setenv("NL_TABLE_LDS", "0")
    tab = _tabs(kind, nk=nk)[0]
    nl.set_eam(tab.f, tab.G, tab.r_min_d, tab.r_max_d, tab.E, tab.P, tab.rho_max)  # (the same tables, the same list)
    assert not nl.eam()["lds_forces"] and not nl.eam()["lds_density"]
    b = _run(nl, qd, ref, dtype)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    monkeypatch.delenv("NL_TABLE_LDS")
    half, qh = _built(q, box, dtype, False, 3.4, kind, nk=nk)
    _run(half, qh, ref, dtype)
    monkeypatch.setenv("NL_TABLE_LDS", "0")
    half.set_eam(tab.f, tab.G, tab.r_min_d, tab.r_max_d, tab.E, tab.P, tab.rho_max)
    _run(half, qh, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_embedding_is_the_pair_table(kind, dtype):
    """E = P = 0: on one full list eam_forces is table_forces bit for bit, pe_i included, and the totals are table_virial's."""
    box, drift = "xyz", True
    nl, qd = _built(_input(box, drift), box, dtype, True, 3.4, kind, embedding=False)
    f, w = nl.eam_forces(qd).cpu().numpy(), nl.eam_virial(qd).cpu().numpy()
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert f.tobytes() == ft.tobytes() and w.tobytes() == wt.tobytes() and np.isfinite(f).all()
    rho = nl.eam_density()[0].cpu().numpy()
    assert _rho_ratio(rho, _ref(box, drift, kind), dtype).max() <= EAM_C_RHO


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box", ["xyz", "tilt"])
def test_the_density_is_a_table_energy(box, dtype):
    """Every table is read through one knot and one read.  One type, and the pair table's U := the density
    table's f on the same r_min, r_max and knots: on one full list rho_i is 2 pe_i of table_forces bit for bit -- the same walk,
    lane order and wave sum, and every term of pe_i is a term of rho_i halved, which is exact: f >= f(R_MAX) = 0.06 on the
    whole table, so no term comes near the underflow of either dtype and no table scale is needed."""
    tab = _tabs("one")[0]
    assert tab.f.min() > 0.05 and (tab.r_min_d, tab.r_max_d, tab.f.shape[1]) == (tab.r_min, tab.r_max, tab.U.shape[1])
    nl, qd = _built(_input(box, box == "tilt"), box, dtype, True, 3.4, "one")
    nl.set_pair_table(tab.F[0], tab.f[0], tab.r_min, tab.r_max)
    nl.eam_forces(qd)
    rho = nl.eam_density()[0].cpu().numpy()
    pe = nl.table_forces(qd)[:, 3].cpu().numpy()
    assert rho.dtype == np.dtype(dtype) and rho.shape == (N,) and np.all(rho > 1.0)
    assert rho.tobytes() == (2 * pe).tobytes()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_a_zero_pair_table(full, dtype):
    box, drift, kind = "tilt", False, "three"
    q = _input(box, drift)
    ref = _refs(q, box, kind, _pairs(box, drift), pair=False)
    assert np.abs(ref["want"][:, :3]).max() > 0.1 and ref["ww"][7] > N
    nl, qd = _built(q, box, dtype, full, 3.4, kind, pair=False)
    _run(nl, qd, ref, dtype)


def _assert_nan_pattern(f, rho, w, ref, dtype):
    """NaN exactly where the reference has it; everybody else within the bound; all 8 totals NaN."""
    f, rho, w = f.cpu().numpy(), rho.cpu().numpy(), w.cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,) and np.isnan(ref["ww"]).all()
    assert np.array_equal(np.isnan(f), np.isnan(ref["want"])) and np.array_equal(np.isnan(rho), np.isnan(ref["rho"]))
    clean = ~np.isnan(ref["want"]).any(axis=1)
    check_lj(f, ref["want"], ref["S"], dtype, c=EAM_C, rows=clean)
    pe_ok = ~np.isnan(ref["want"][:, 3])  # (a partner's force is NaN, its energy is not)
    assert np.all(np.abs(f[pe_ok, 3].astype(np.float64) - ref["want"][pe_ok, 3]) <= EAM_C * lj_unit(dtype) * ref["S"][pe_ok, 3])
    ok = ~np.isnan(ref["rho"])
    assert _rho_ratio(rho, ref, dtype)[ok].max() <= EAM_C_RHO


def _beyond_rho_max(r_max_d):
    """(rho_max, reference, the particle a above rho_max, its partners within r_max_d) of test_a_density_beyond_rho_max."""
    box, drift, kind = "xyz", False, "one"
    q, pairs = _input(box, drift), _pairs(box, drift)
    top = np.sort(_refs(q, box, kind, pairs, r_max_d=r_max_d)["rho"])[-2:]
    assert top[1] - top[0] > 1e-3 * top[1]
    rho_max = float(0.5 * (top[0] + top[1]))
    ref = _refs(q, box, kind, pairs, rho_max=rho_max, r_max_d=r_max_d)
    a = int(np.argmax(ref["rho"]))
    I, J, _, r2 = eam_list_pairs(_tabs(kind)[0], pairs)
    return rho_max, ref, a, J[(I == a) & (r2 < r_max_d ** 2)], J[I == a]


def test_a_nan_fp_stops_at_r_max_d():
    """The reference of test_a_density_beyond_rho_max: NaN energy for the one particle, NaN forces for it and exactly its partners
    within r_max_d -- with r_max_d = R_SHORT fewer than its partners in the list, so a kernel that multiplied a NaN fp by G = 0
    beyond r_max_d would be told apart."""
    for r_max_d in (R_MAX, R_SHORT):
        _, ref, a, near, listed = _beyond_rho_max(r_max_d)
        nan_f, nan_e = np.isnan(ref["want"][:, 0]), np.isnan(ref["want"][:, 3])
        assert np.array_equal(np.flatnonzero(nan_e), [a]) and np.array_equal(np.flatnonzero(nan_f), np.unique(np.append(near, a)))
        assert np.isnan(ref["fp"]).sum() == 1 and not np.isnan(ref["rho"]).any() and np.isnan(ref["ww"]).all()
        assert (len(near) < len(listed) - 10) == (r_max_d == R_SHORT) and len(near) > 20


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("r_max_d", [R_MAX, R_SHORT])
def test_a_density_beyond_rho_max(r_max_d, full, dtype):
    """rho_max between the largest and the second largest density: that one particle has no F' -- NaN in its own force and
    energy, in the forces (not the energies) of exactly its partners within r_max_d, and in all 8 totals.  With r_max_d = R_SHORT
    the list and the pair table reach further than the density: the partners between R_SHORT and R_MAX stay finite."""
    rho_max, ref, a, _, _ = _beyond_rho_max(r_max_d)
    nl, qd = _built(_input("xyz", False), "xyz", dtype, full, 2.5, "one", rho_max=rho_max, r_max_d=r_max_d)
    f, w = nl.eam_forces(qd), nl.eam_virial(qd)
    rho, fp = nl.eam_density()
    assert np.array_equal(np.flatnonzero(np.isnan(fp.cpu().numpy())), [a])
    _assert_nan_pattern(f, rho, w, ref, dtype)


def _unequal(which, kind):
    """The tables' keywords, the reference and its pair counts for r_max_d != r_max: "density short" (r_max_d = R_SHORT < r_max =
    R_MAX) and "pair short" (the other way round), on the drifted tilted box."""
    box, drift = "tilt", True
    kw = dict(r_max_d=R_SHORT) if which == "density short" else dict(r_max_pair=R_SHORT)
    q, pairs = _input(box, drift), _pairs(box, drift)
    tab, types, rc_ab = _tabs(kind, **kw)
    r2 = eam_list_pairs(tab, pairs, types, None if rc_ab is None else rc_ab(3.4))[3]
    return kw, _refs(q, box, kind, pairs, **kw), (r2 < R_SHORT ** 2).sum() / 2, len(r2) / 2


def test_unequal_ranges_are_told_apart():
    """No pair lies within 2^-17 (relative, r^2) of R_SHORT, and n_in of the reference counts the pairs within the LONGER of the
    two ranges, in = in_phi || in_d: many more than within the shorter one, which is what either test alone would count."""
    for box, drift in (("tilt", True), ("xyz", False)):
        d = _pairs(box, drift)[2]
        assert not np.any(np.abs((d * d).sum(axis=1) / R_SHORT ** 2 - 1.0) < 2.0 ** -17)
    for which in ("density short", "pair short"):
        for kind in KINDS:
            _, ref, n_short, n_long = _unequal(which, kind)
            assert ref["ww"][7] == n_long > n_short + 10000 and np.isfinite(ref["want"]).all()
            assert np.all((ref["rho"] > 0) & (ref["rho"] < RHO_MAX[kind]))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("which", ["density short", "pair short"])
def test_unequal_ranges(which, full, dtype):
    """r_max_d != r_max, both ways, one type and three: forces, energies, rho and the totals against the reference, n_in exactly
    the pairs within the longer range (in = in_phi || in_d, which also decides the half list's reaction)."""
    for kind in KINDS:
        kw, ref, _, _ = _unequal(which, kind)
        nl, qd = _built(_input("tilt", True), "tilt", dtype, full, 2.5, kind, **kw)
        _run(nl, qd, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_a_pair_below_the_density_table(full, dtype):
    """One particle moved to 0.5 from its neighbour: below r_min_d = 0.85, inside the pair table (sampled from 0.4 here).  Both
    densities are NaN, and from there both particles' forces and energies, their partners' forces and all 8 totals."""
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
    assert np.array_equal(np.flatnonzero(np.isnan(ref["rho"])), sorted((a, b))) and np.isnan(ref["want"][:, 3]).sum() == 2
    assert np.isnan(ref["want"][:, 0]).sum() > 20
    nl, qd = _built(q, box, dtype, full, 2.5, kind, r_min_pair=0.4)
    f, w = nl.eam_forces(qd), nl.eam_virial(qd)
    _assert_nan_pattern(f, nl.eam_density()[0], w, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,kind", [("xyz", "one"), ("tilt", "three")])
def test_reuse_within_the_skin(box, kind, full, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants; no extra build."""
    contract.reuse_within_the_skin(EAM, box, kind, full, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """A capture before the first call is NL_ERR_STATE (the scratch cannot be allocated); after one synchronous call one graph
    holds the copy of the positions, the update, the forces and the totals, replayed at two position sets."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()

    def before(nl, qd, fd, wd):
        nl.table_virial(qd, wait=False)  # (the totals' scratch exists: what is missing below is the EAM scratch)
        nl.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0):
            for call, o in ((nl.eam_forces, fd), (nl.eam_virial, wd)):
                with pytest.raises(NLError) as e:
                    call(qd, wait=False, out=o)
                assert e.value.code == NL_ERR_STATE
            nl.table_forces(qd, wait=False, out=fd)
        nl.eam_forces(qd)  # synchronous, outside a capture: allocates

    def after(nl, replay):
        # tables of the same size set afterwards keep the device buffer: the next replay computes with them
        tab = _tabs("one", embedding=False)[0]
        nl.set_eam(tab.f, tab.G, tab.r_min_d, tab.r_max_d, tab.E, tab.P, tab.rho_max)
        fd, wd = replay()
        q1, pairs1 = _moved("xyz")
        _check(fd, nl.eam_density()[0], wd, _refs(q1, "xyz", "one", pairs1, embedding=False), np.float32)

    contract.captured(EAM, full, before, after)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces, densities and totals, NL_ERR_CAPACITY
    at synchronize; after the synchronous repeat all are finite."""
    def set_tables(nl):
        fs, dfs, Fs, dFs = eam_functions(1)
        nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, R_MAX, NK), 1e-3, R_MAX)  # (a uniform random box has close pairs)
        f, G, E, P = eam.sample(fs[0], dfs[0], Fs[0], dFs[0], 1e-3, R_MAX, NK, 400.0, NK)
        nl.set_eam(f, G, 1e-3, R_MAX, E, P, 400.0)

    def prepare(nl, qd):
        nl.update(qd, sync=True)
        nl.eam_virial(qd)  # (the scratch of both kinds)

    contract.failed_list(EAM, set_tables, prepare)


@gpu
@pytest.mark.parametrize("off", [32, 64])
@pytest.mark.parametrize("full", [False, True])
def test_both_offset_widths(full, off):
    contract.both_offset_widths(EAM, full, off)


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
    calls = contract.entry_calls(EAM, lib, fd, out)
    set_one = lambda t=tab: nl.set_eam(t.f, t.G, t.r_min_d, t.r_max_d, t.E, t.P, t.rho_max)  # noqa: E731
    # nothing set; only the pair table; only the EAM tables
    assert nl.eam() is None and lib.nl_get_eam(nl._h, *([None] * 8)) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for have_pair, have_eam in ((False, False), (True, False), (False, True)):
        nl.set_pair_table(F, U, R_MIN, R_MAX) if have_pair else nl.clear_pair_table()
        set_one() if have_eam else nl.clear_eam()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    p = C.c_void_p()
    assert lib.nl_eam_get_density(nl._h, C.byref(p), C.byref(p), C.byref(C.c_int32())) == NL_ERR_STATE  # (no call yet)
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    want = nl.eam_virial(qd).cpu().numpy()  # (a full list: reproducible bit for bit)
    assert np.isfinite(want).all()
    # the setter's arguments: each refused, and the tables that were set are kept
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    f, G, E, P = tab.f[0].copy(), tab.G[0].copy(), tab.E[0].copy(), tab.P[0].copy()
    bad = {}
    for name, arr, v in (("f", f, np.inf), ("G", G, np.nan), ("E", E, -np.inf), ("P", P, np.nan)):
        bad[name] = arr.copy()
        bad[name][5] = v
    big = np.zeros(4097)
    rm = RHO_MAX["one"]
    good = dict(nt=1, nd=NK, lo=R_MIN, hi=R_MAX, f=f, G=G, ne=NK, rm=rm, E=E, P=P)
    keep = []  # (the arrays behind the pointers)

    def args(**kw):
        a = dict(good, **kw)
        ptrs = {k: None if a[k] is None else dp(a[k]) for k in "fGEP"}
        keep.append(ptrs)
        return a["nt"], a["nd"], a["lo"], a["hi"], ptrs["f"], ptrs["G"], a["ne"], a["rm"], ptrs["E"], ptrs["P"]

    for kw in (dict(f=None), dict(G=None), dict(E=None), dict(P=None), dict(nd=1), dict(ne=1), dict(nd=-2), dict(nd=4097, f=big, G=big),
               dict(ne=4097, E=big, P=big), dict(lo=0.0), dict(lo=-1.0), dict(lo=R_MAX), dict(hi=np.inf), dict(lo=np.nan), dict(rm=0.0),
               dict(rm=-1.0), dict(rm=np.inf), dict(rm=np.nan), dict(nt=0), dict(nt=33), dict(f=bad["f"]), dict(G=bad["G"]), dict(E=bad["E"]),
               dict(P=bad["P"])):
        assert lib.nl_set_eam(nl._h, *args(**kw)) == NL_ERR_ARG, kw.keys()
        assert nl.eam()["nknots_d"] == NK and nl.eam()["rho_max"] == rm
    assert lib.nl_set_eam(None, *args()) == NL_ERR_ARG
    assert nl.eam_virial(qd).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(TypeError):
        nl.set_eam(f, G[:-1], R_MIN, R_MAX, E, P, rm)
    with pytest.raises(TypeError):
        nl.set_eam(tab3.f, tab3.G, R_MIN, R_MAX, E, P, rm)  # 3 density slots, 1 embedding slot
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_one)
    # reach of the density table (the pair table stays at 2.5)
    fs, dfs, Fs, dFs = eam_functions(1)

    def set_r_max(r_max):
        t = eam.sample(fs[0], dfs[0], Fs[0], dFs[0], R_MIN, r_max, NK, 60.0, NK)
        nl.set_eam(t[0], t[1], R_MIN, r_max, t[2], t[3], 60.0)

    contract.reach(EAM, nl, qd, set_r_max)
    # ... and of the pair table
    set_one()
    nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, 2.7, NK), R_MIN, 2.7)
    nl.eam_forces(qd)
    with pytest.raises(NLError) as e:
        nl.eam_forces(qd, wait=False)
    assert e.value.code == NL_ERR_ARG
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    contract.clearing(EAM, nl, qd, set_one, lambda: lib.nl_set_eam(nl._h, *args(nd=0)))
    # several types: a type table of that ntypes, a pair table of 1 or ntypes types
    contract.several_types(EAM, nl, qd, types, set_one, lambda: set_one(tab3))  # (a pair table of one type under three density slots)
    nl.set_pair_table(tab3.F, tab3.U, R_MIN, R_MAX)
    assert torch.isfinite(nl.eam_forces(qd)).all()
    # nl_initialize drops the scratch; the next call allocates it again, for more particles
    nl.clear_type_cutoffs()
    set_one()
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    nl.Initialize(2 * N)
    assert lib.nl_eam_get_density(nl._h, C.byref(p), C.byref(p), C.byref(C.c_int32())) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    _run(nl, qd, _ref("open", False, "one"), np.float32)

    # n == 0
    def set_tables(empty):
        empty.set_pair_table(F, U, R_MIN, R_MAX)
        empty.set_eam(tab.f, tab.G, R_MIN, R_MAX, tab.E, tab.P, rm)

    contract.no_particles(EAM, lib, False, set_tables, qd, fd, out)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_slab_lists_are_refused(full):
    """A slab build, with and without nl_set_local_ids: NL_ERR_STATE from all four calls (fp of the ghosts is a halo exchange of
    the caller's)."""
    contract.slab_lists_are_refused(EAM, full)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_distributed_lists_are_refused(full):
    """A distributed build of a world of one (nl_make_list_distributed: the whole box, the global ids in w): its list holds
    caller ids, and all four calls are NL_ERR_STATE, wait and enqueue."""
    contract.distributed_lists_are_refused(EAM, full)

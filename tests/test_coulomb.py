"""Per-particle charges (nl_set_coulomb_table, nl_coul_forces, nl_coul_virial and their enqueue variants) against an O(N^2)
float64 evaluation of the rule of include/nl_hip.h, with an error bound per particle and per component, and the samplers of
md_neighbor_list_amd.coulomb against their own derivatives.

Contract tested (include/nl_hip.h, nl_set_coulomb_table):
  * |got - want| <= COUL_C u S for every particle and each of fx, fy, fz, pe on its own, and <= COUL_CW u S for each of the 7
    sums of the totals, n_in exact: want the float64 sum of tests.util_coulomb coul_reference (pair_table.interpolate on the
    pair table plus q_i q_j coulomb.interpolate on the charge table; no list), S the uncancelled sums of both tables' terms
    with the conditioning of s on the rounding of r2;
  * zero charges give nl_table_forces, doubled charges four times the charge term, exactly;
  * a pair below r_min_c gives NaN to exactly its two particles and to all 8 totals, two neutral particles included;
  * the LDS and the global path compute the same bits;
  * what tests.consumer_contract states for every table-driven consumer.

The constants are not fitted to the kernel.  COUL_C and COUL_CW are 4 x the largest |emulated - want| / (u S) that a numpy
emulation of the rule reaches (tests.util_coulomb coul_emulate: one rounding per operation, no FMA, every particle's terms
summed in a random order; coul_virial_emulate: the kernels' own summation tree in both position types) over the inputs of
util_coulomb.EMULATED, three summation orders each; test_emulation_gives_c recomputes both maxima.  The factor 4 covers the
GPU's other summation order within a row.

The excluded-pair term of Ewald sums (a second table over the pairs nl_set_exclusions removed) is not built and has no tests.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import coulomb, pair_table
from tests import consumer_contract as contract
from tests import util_coulomb as uc
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _handle, _off_the_band, _pair_tab, _tab, _tdt, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_unit
from tests.util_coulomb import COUL_C, COUL_CW, EMULATED, EMULATED_MAX, EMULATED_MAX_W, KINDS, NKC
from tests.util_table import morse
from tests.virial_util import check_virial, virial_ratio

RC_LISTS = (2.5, 3.4)
GRID = (R_MIN, R_MAX, NKC)
LDS_BYTES = 65280  # NL_TABLE_LDS_BYTES of include/nl_hip.h (test_lds_and_global_paths reads it there)
ENTRY = ("nl_coul_forces", "nl_coul_forces_enqueue", "nl_coul_virial", "nl_coul_virial_enqueue")


# --------------------------------------------------------------------------------------------------- CPU: the samplers
def _samplers():
    rc = R_MAX
    return {
        "ewald_real": lambda *g, **kw: coulomb.ewald_real(0.4, *g, **kw),
        "dsf": lambda *g, **kw: coulomb.dsf(0.3, rc, *g, **kw),
        "wolf": lambda *g, **kw: coulomb.wolf(0.3, rc, *g, **kw),
        "reaction_field": lambda *g, **kw: coulomb.reaction_field(78.5, rc, *g, **kw),
        "reaction_field_conducting": lambda *g, **kw: coulomb.reaction_field(float("inf"), rc, *g, **kw),
        "debye": lambda *g, **kw: coulomb.debye(0.7, *g, **kw),
        "shifted": lambda *g, **kw: coulomb.shifted(rc, *g, **kw),
    }


@pytest.mark.parametrize("name", sorted(_samplers()))
def test_sampler_k_is_the_derivative_of_its_c(name):
    """K = -C'(r) / r by central differences of the sampler's own C: a table of two knots at r -+ h gives C there (the grid
    puts knots at r_min and r_max).  C has bounded third derivatives on [0.85, 2.5]: h = 1e-5 leaves h^2 C''' / 6 ~ 1e-10."""
    sample = _samplers()[name]
    K, Cv = sample(*GRID)
    r = pair_table.knots(*GRID)
    assert K.shape == Cv.shape == (NKC,) and K.dtype == Cv.dtype == np.float64 and np.isfinite(K).all() and np.isfinite(Cv).all()
    h = 1e-5
    for k in range(0, NKC, 37):
        (_, lo), (_, hi) = (sample(r[k] + s * h, r[k] + s * h + 1.0, 2) for s in (-1.0, 1.0))
        assert abs(-(hi[0] - lo[0]) / (2 * h) / r[k] - K[k]) <= 1e-8 * (abs(K[k]) + abs(Cv[k]) / r[k] ** 2) + 1e-9, (name, k)
    K3, C3 = sample(*GRID, prefactor=3.0)
    assert np.array_equal(K3, 3.0 * K) and np.array_equal(C3, 3.0 * Cv)


def test_sampler_identities():
    r = pair_table.knots(*GRID)
    K0, C0 = coulomb.ewald_real(0.0, *GRID)  # alpha -> 0: plain Coulomb, which is `shifted` without the shift
    Ks, Cs = coulomb.shifted(R_MAX, *GRID)
    assert np.allclose(K0, Ks, rtol=1e-14, atol=0) and np.allclose(C0, Cs + 1.0 / R_MAX, rtol=1e-14, atol=0) and np.allclose(C0, 1.0 / r, rtol=1e-14, atol=0)
    assert Cs[-1] == 0.0
    Kd, Cd = coulomb.dsf(0.3, R_MAX, *GRID)  # force and energy vanish at r_cut (the last knot)
    assert abs(Kd[-1]) <= 1e-15 and abs(Cd[-1]) <= 1e-15 and Kd[0] > 0.5 and Cd[0] > 0.1
    Kw, Cw = coulomb.wolf(0.3, R_MAX, *GRID)
    assert abs(Cw[-1]) <= 1e-15 and np.array_equal(Kw, coulomb.ewald_real(0.3, *GRID)[0])
    assert abs(coulomb.reaction_field(78.5, R_MAX, *GRID)[1][-1]) <= 1e-15
    assert abs(coulomb.reaction_field(float("inf"), R_MAX, *GRID)[0][-1]) <= 1e-15  # conducting: the force vanishes too
    K, Cv = coulomb.ewald_real(0.4, *GRID)
    x = np.linspace(R_MIN ** 2, R_MAX ** 2, 1001)[:-1]
    kc, cc, inn = coulomb.interpolate(K, Cv, R_MIN, R_MAX, x)
    assert inn.all() and np.array_equal(kc[0], K[0]) and np.array_equal(cc[0], Cv[0])
    exact = np.array([math.erfc(0.4 * v) / v for v in np.sqrt(x)])
    assert np.abs(cc - exact).max() < 1e-4  # D^2 max |C_xx| / 8 = 2.5e-5 at 512 knots
    out = coulomb.interpolate(K, Cv, R_MIN, R_MAX, np.array([0.0, 0.5 * R_MIN ** 2, R_MAX ** 2]))
    assert np.isnan(out[0][1]) and out[0][0] == 0.0 and out[1][2] == 0.0 and list(out[2]) == [False, True, False]


# --------------------------------------------------------------------------------------------------- CPU: the checker
def test_inputs():
    for kind in KINDS:
        q = uc.charges(kind)  # (asserts the zero sum, |q| >= Q_MIN and float32 values)
        assert q.shape == (N,) and (q > 0).sum() == N // 2
    assert set(np.unique(uc.charges("salt"))) == {-1.0, 1.0}
    idx = np.arange(N).reshape(LJ_M, LJ_M, LJ_M)
    assert np.all(uc.charges("salt")[idx[1:].ravel()] == -uc.charges("salt")[idx[:-1].ravel()])  # neighbours along x are unlike
    K, Cv = uc.coul_tab()
    assert K.shape == (NKC,) and NKC != NK and np.isfinite(K).all() and np.isfinite(Cv).all()
    assert K[-1] * R_MAX > 0.3 and Cv[-1] > 0.2  # the charge term does not vanish at r_max
    m = uc.model("typed3")
    assert m.F.shape == (6, NK) and m.rc_ab[0, 2] == 0 and set(m.types.tolist()) == {0, 1, 2}


def test_reference_is_the_gradient_of_its_energy():
    """coul_reference's forces against the central difference of its own total energy, tilted and periodic, two types, random
    charges.  Both potentials are linear in r^2 (U = b (r_max^2 - r^2), C = c (r_max^2 - r^2)): both tables interpolate them
    exactly and they vanish at r_max, so the energy has no jump there and the forces are its gradient to rounding."""
    rng = np.random.default_rng(3)
    m_, a = 5, 1.125
    box6, mask = (m_ * a, m_ * a, m_ * a, a, -a, 2 * a), 7
    g = np.stack(np.meshgrid(*(np.arange(m_),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (g + 0.5) * a + rng.uniform(-0.1, 0.1, size=g.shape)
    r_max, h = 1.8, 1e-5
    types = rng.integers(0, 2, size=len(q))
    rows = [pair_table.sample(lambda r, v=v: v * (r_max ** 2 - r * r), lambda r, v=v: -2.0 * v * r, 0.5, r_max, 64) for v in (1.0, 1.7, 0.6)]
    F, U = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    K, Cv = pair_table.sample(lambda r: 0.9 * (r_max ** 2 - r * r), lambda r: -1.8 * r, 0.4, r_max, 33)
    m = uc.Model(F, U, 0.5, r_max, K, Cv, 0.4, r_max, rng.uniform(-1.0, 1.0, size=len(q)), types)
    (want, S), (w, SW) = uc.coul_reference(q, box6, mask, m)
    for i in range(4):
        for c in range(3):
            e = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                e.append(uc.coul_reference(p, box6, mask, m)[0][0][:, 3].sum())
            fd = -(e[0] - e[1]) / (2 * h)
            assert abs(fd - want[i, c]) <= 1e-6 * S[i, c], (i, c, fd, want[i, c])
    assert np.abs(want[:, :3].sum(axis=0)).max() <= 1e-12 * S[:, :3].sum()  # Newton's third law in the reference
    assert abs(w[6] - want[:, 3].sum()) <= 1e-12 * SW[6] and w[7] > len(q)
    neutral = uc.Model(F, U, 0.5, r_max, K, Cv, 0.4, r_max, np.zeros(len(q)), types)  # no charges: the pair table alone
    from tests.util_table import table_reference

    assert np.array_equal(uc.coul_reference(q, box6, mask, neutral)[0][0], table_reference(q, box6, mask, F, U, 0.5, r_max, types=types)[0])


def test_emulation_gives_c():
    """COUL_C and COUL_CW = 4 x the largest |emulated - want| / (u S) of a numpy emulation of the kernel's arithmetic (never
    the kernel) against the float64 reference: per particle and component in fp32, the totals in both position types."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    for box, drift, kind in EMULATED:
        box6, mask = LJ_BOXES[box]
        m = uc.model(kind)
        (want, S), (ww, SW) = uc.ref(box, drift, kind)
        I, J = uc.listed(m, *_pairs(box, drift)[:2])
        q = _input(box, drift)
        vals = {T: uc.coul_emulate_pairs(q, box6, mask, m, T, (I, J)) for T in DTYPES}
        for order in range(3):
            rng = np.random.default_rng(100 + order)
            f = uc.coul_emulate(q, box6, mask, m, np.float32, rng, (I, J))
            r = lj_ratio(f, want, S, np.float32).max(axis=0)
            rw = []
            for T in DTYPES:  # (the totals are summed in double whatever T is: in fp64 that sum is the error)
                w = uc.coul_virial_emulate(N, I, vals[T], rng)
                assert w[7] == ww[7]
                rw.append(virial_ratio(w, ww, SW, T))
            print(box, drift, kind, order, r.round(2), rw[0].round(3), rw[1].round(3))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, np.maximum(*rw))
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX <= COUL_C / 4
    assert worst_w.max() <= EMULATED_MAX_W <= COUL_CW / 4
    assert EMULATED_MAX - worst.max() < 0.01 and EMULATED_MAX_W - worst_w.max() < 0.001  # the constants are the measured maxima


def _assert_sharp(refs, kind):
    (_, S), _ = refs
    Fm, Um = uc.weakest(uc.model(kind))
    u = lj_unit(np.float32)
    assert np.all(COUL_C * u * S[:, :3].max(axis=1) <= 0.25 * Fm), (COUL_C * u * S[:, :3].max() / Fm)
    assert np.all(COUL_C * u * S[:, 3] <= 0.25 * Um), (COUL_C * u * S[:, 3].max() / Um)


def test_bound_is_sharp():
    """On every input COUL_C u S stays below a quarter of what the weakest single charged pair at r_max_c gives a component
    through its charge term alone (|q| >= 0.5: the float64 reference and the charge sets decide this, no kernel)."""
    seen = 0
    for box, drift in CASES:
        for kind in KINDS:
            _assert_sharp(uc.ref(box, drift, kind), kind)
            seen += 1
    for box in ("xyz", "tilt"):
        for kind in KINDS:
            _assert_sharp(uc.moved_ref(box, kind), kind)
    assert seen == 18


def test_wrong_results_are_rejected():
    """check_lj under the fp32 bound refuses every mistake of util_coulomb.DEFECTS made in the emulator, on both charge sets:
    q_j for q_i q_j, the row's charge for the partner's, C and K swapped, the charge term left out of pe, a half list's
    reaction without its charge factor.  The emulator without a defect passes."""
    for box, drift, kind in (("xyz", False, "salt"), ("tilt", True, "typed3")):
        box6, mask = LJ_BOXES[box]
        m = uc.model(kind)
        (want, S), _ = uc.ref(box, drift, kind)
        pairs = uc.listed(m, *_pairs(box, drift)[:2])
        q = _input(box, drift)
        rng = np.random.default_rng(5)
        check_lj(uc.coul_emulate(q, box6, mask, m, np.float64, rng, pairs), want, S, np.float32, c=COUL_C)
        for defect in uc.DEFECTS:
            with pytest.raises(AssertionError):
                check_lj(uc.coul_emulate(q, box6, mask, m, np.float64, rng, pairs, defect), want, S, np.float32, c=COUL_C)


# ------------------------------------------------------------------------------------------------------ GPU helpers
class _WithCharges:
    """The library as tests.consumer_contract calls it -- fn(handle, q, stride, out, stream) -- with the charge pointer put in
    for the four entry points; every other call, and a call that brings its own charge pointer, goes through unchanged."""

    def __init__(self, lib, charges):
        self.__dict__.update(_lib=lib, _charges=charges)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY:
            return fn
        return lambda *a: fn(*a) if len(a) == 6 else fn(*a[:3], self._charges.data_ptr(), *a[3:])


def _charge_tensor(nl, values):
    return _torch().from_numpy(np.array(values, dtype=np.float64)).to(nl.dtype).cuda()


def _set(nl, kind, rc, nk=NK, nkc=NKC, order=None):
    """The kind's pair table (and type table at the list's cut-off), the charge table and the charges onto an initialised
    handle.  order: the rows of a slab build."""
    F, U, types, rc_ab = uc.pair_tab(kind, nk)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    nl.set_coulomb_table(*uc.coul_tab(nkc), R_MIN, R_MAX)
    q = uc.charges(kind)
    nl.set_charges(_charge_tensor(nl, q if order is None else q[order]))
    if not isinstance(nl._lib, _WithCharges):
        nl._lib = _WithCharges(nl._lib, nl._charges)


def _check(f, w, refs, dtype, rows=None):
    (want, S), (ww, SW) = refs
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, want, S, dtype).max(axis=0).round(2), virial_ratio(w, ww, SW, dtype).round(2))
    check_lj(f, want, S, dtype, c=COUL_C, rows=rows)
    if rows is None:
        check_virial(w, ww, SW, dtype, c=COUL_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (COUL_C + COUL_CW) * lj_unit(dtype) * SW[6]
    return f, w


COUL = contract.Consumer(
    forces="coul_forces", virial="coul_virial", scratch="coul_virial", clear="clear_coulomb_table", info="coulomb_table_info", entry=ENTRY,
    set=_set, kinds=KINDS, ref=uc.ref, moved_ref=uc.moved_ref, extra=lambda nl: (),
    check=lambda f, w, x, refs, dtype, rows=None: _check(f, w, refs, dtype, rows), half_lists=True, local_slabs=True)
_built = functools.partial(contract.built, COUL)
gpu = pytest.mark.gpu


def _refs(q, box, m, pairs):
    box6, mask = LJ_BOXES[box]
    return uc.coul_reference(q, box6, mask, m, pairs)


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x both kinds (one type and rock salt; three types and random charges) x list kind x
    dtype; the list cut-off, the offset width and q_stride rotate through the cases.  Two calls of the totals are bit-identical."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, kind in enumerate(KINDS):
        k = case + p + (1 if full else 0)
        rc, off, stride = RC_LISTS[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        nl, qd = _built(q, box, dtype, full, rc, kind, off, stride)
        assert nl.build_info()["offset_bits"] == off and qd.shape[1] == stride
        lds = (np.atleast_2d(uc.pair_tab(kind)[0]).size + NKC) * 4 * np.dtype(dtype).itemsize <= LDS_BYTES  # (typed3: 6 slots, global)
        assert nl.coulomb_table_info() == dict(nknots=NKC, r_min=R_MIN, r_max=R_MAX, lds=lds)
        f, w = nl.coul_forces(qd), nl.coul_virial(qd)
        assert f.shape == (N, 4) and f.dtype == _tdt(dtype) and w.shape == (8,) and w.dtype == _torch().float64
        _, w = _check(f, w, uc.ref(box, drift, kind), dtype)
        assert w.tobytes() == nl.coul_virial(qd).cpu().numpy().tobytes() and len(w.tobytes()) == 64


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "typed3"), ("xyz", False, "salt")])
def test_zero_charges_are_the_pair_table(box, drift, kind, dtype):
    """A full list, r_max_c == r_max, every charge 0: forces, energies and the 7 sums equal nl_table_forces' and
    nl_table_virial's by value (0 kc adds nothing; == and not bits: the sign of a zero may differ), n_in as well."""
    nl, qd = _built(_input(box, drift), box, dtype, True, 3.4, kind)
    zero = _torch().zeros(N, dtype=_tdt(dtype), device="cuda")
    f, w = nl.coul_forces(qd, charges=zero).cpu().numpy(), nl.coul_virial(qd, charges=zero).cpu().numpy()
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert np.isfinite(ft).all() and np.abs(ft).max() > 0.1 and wt[7] > 10 * N
    assert np.all(f == ft) and np.all(w == wt)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "typed3"), ("open", False, "salt")])
def test_doubled_charges_scale_by_four(box, drift, kind, dtype):
    """A full list and a pair table of zeros: charges x 2 give forces, energies and the 7 sums x 4 exactly (powers of two go
    through every product and every sum of one fixed order), and the same n_in."""
    torch = _torch()
    nl, qd = _built(_input(box, drift), box, dtype, True, 2.5, kind)
    F = uc.pair_tab(kind)[0]
    nl.set_pair_table(np.zeros_like(F), np.zeros_like(F), R_MIN, R_MAX)
    q1 = _charge_tensor(nl, uc.charges(kind))
    f1, w1 = nl.coul_forces(qd, charges=q1).cpu().numpy(), nl.coul_virial(qd, charges=q1).cpu().numpy()
    f2, w2 = nl.coul_forces(qd, charges=2 * q1).cpu().numpy(), nl.coul_virial(qd, charges=2 * q1).cpu().numpy()
    assert np.isfinite(f1).all() and np.abs(f1).max() > 0.1 and torch.is_tensor(q1)
    assert np.array_equal(f2, 4 * f1) and np.array_equal(w2[:7], 4 * w1[:7]) and w2[7] == w1[7] > 10 * N


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "typed3"), ("xyz", False, "salt")])
def test_half_and_full_agree(box, drift, kind, dtype):
    refs = uc.ref(box, drift, kind)
    got = {}
    for full in (False, True):
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, kind)
        got[full] = _check(nl.coul_forces(qd), nl.coul_virial(qd), refs, dtype)
    u = lj_unit(dtype)
    assert np.all(np.abs(got[False][0].astype(np.float64) - got[True][0]) <= 2 * COUL_C * u * refs[0][1])
    assert np.all(np.abs(got[False][1][:7] - got[True][1][:7]) <= 2 * COUL_CW * u * refs[1][1])
    assert got[False][1][7] == got[True][1][7] == refs[1][0][7]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,nk", [("salt", NK), ("typed3", 128)])
def test_lds_and_global_paths(kind, nk, dtype, monkeypatch):
    """A charge table set under NL_TABLE_LDS=0 makes the calls read both tables from global memory.  On one list the two paths
    give the same bits: full-list forces and the totals of both list kinds; half-list forces within the bound.  Two tables
    that do not fit NL_TABLE_LDS_BYTES together take the global path by themselves."""
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    lds_bytes = int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1))
    knot = 4 * np.dtype(dtype).itemsize
    assert lds_bytes == LDS_BYTES and (np.atleast_2d(uc.pair_tab(kind, nk)[0]).size + NKC) * knot <= lds_bytes  # staged unless switched off
    box, drift = "tilt", True
    refs = _refs(_input(box, drift), box, uc.model(kind, nk), _pairs(box, drift))
    for full in (False, True):
        monkeypatch.delenv("NL_TABLE_LDS", raising=False)
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, kind, nk=nk)
        assert nl.coulomb_table_info()["lds"]
        lds = _check(nl.coul_forces(qd), nl.coul_virial(qd), refs, dtype)
        monkeypatch.setenv("NL_TABLE_LDS", "0")
        nl.set_coulomb_table(*uc.coul_tab(), R_MIN, R_MAX)  # (the same table, the same list: the other path)
        assert not nl.coulomb_table_info()["lds"]
        glo = _check(nl.coul_forces(qd), nl.coul_virial(qd), refs, dtype)
        assert lds[1].tobytes() == glo[1].tobytes() and len(glo[1].tobytes()) == 64
        if full:
            assert lds[0].tobytes() == glo[0].tobytes()
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nkc = 3584  # with the 1024 knots of the pair table: 4608 knots, 72 KiB in fp32 -- beyond LDS together, each within it alone
    assert (NK + nkc) * knot > lds_bytes
    big = uc.model("salt", NK, nkc)
    nl, qd = _built(_input(box, drift), box, dtype, True, 3.4, "salt", nkc=nkc)
    assert not nl.coulomb_table_info()["lds"]
    _check(nl.coul_forces(qd), nl.coul_virial(qd), _refs(_input(box, drift), box, big, _pairs(box, drift)), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("neutral", [False, True])
def test_a_pair_below_the_charge_table(neutral, full, dtype):
    """One particle moved to 0.5 from its neighbour, inside a pair table that starts at 0.4 and below r_min_c = 0.85: NaN in
    exactly those two particles' forces and energies, 8 NaN totals, everybody else within the bound.  neutral: both particles
    carry no charge -- the pair has no value all the same."""
    box = "xyz"
    box6, mask = LJ_BOXES[box]
    q = _input(box, False).copy()
    a = int(np.ravel_multi_index((6, 7, 5), (LJ_M,) * 3))
    b = int(np.ravel_multi_index((7, 7, 5), (LJ_M,) * 3))
    q[b, :3] = (q[a, :3] + [0.5, 0.0, 0.0]).astype(np.float32)
    pairs = lj_pairs(q, box6, mask, R_MAX * (1 + 2.0 ** -16))
    assert _off_the_band(None, box6, mask, pairs)
    r = np.sqrt((pairs[2] ** 2).sum(axis=1))
    assert (r < R_MIN).sum() == 2 and abs(r.min() - 0.5) < 1e-6  # the one pair, in both orders
    chg = uc.charges("salt").copy()
    if neutral:
        chg[[a, b]] = 0.0
    F, U = _pair_tab(1, 0.4, R_MAX, NK)
    m = uc.Model(F, U, 0.4, R_MAX, *uc.coul_tab(), R_MIN, R_MAX, chg)
    refs = _refs(q, box, m, pairs)
    nans = np.isnan(refs[0][0]).all(axis=1)
    assert np.array_equal(np.flatnonzero(nans), sorted((a, b))) and np.isnan(refs[1][0]).all()
    nl, qd = _built(q, box, dtype, full, 2.5, "salt")
    nl.set_pair_table(F, U, 0.4, R_MAX)
    assert _torch().isfinite(nl.table_forces(qd)).all()  # (the pair table has a value there)
    cd = _charge_tensor(nl, chg)
    f, w = nl.coul_forces(qd, charges=cd).cpu().numpy(), nl.coul_virial(qd, charges=cd).cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,)
    assert np.array_equal(np.isnan(f), np.repeat(nans[:, None], 4, axis=1))
    check_lj(f, *refs[0], dtype, c=COUL_C, rows=~nans)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,kind", [("xyz", "salt"), ("tilt", "typed3")])
def test_reuse_within_the_skin(box, kind, full, dtype):
    contract.reuse_within_the_skin(COUL, box, kind, full, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """One graph holds the copy of the positions, the update, the forces and the totals; replayed at two position sets.  The
    charges are read, not copied: changed in place they change the next replay; and a charge table of the same size set
    afterwards keeps the device buffer, so the next replay computes with it."""
    def before(nl, qd, fd, wd):
        nl.coul_virial(qd, wait=False, out=wd)  # once before the capture: the scratch exists
        nl.synchronize()

    def after(nl, replay):
        box6, mask = LJ_BOXES["xyz"]
        q, pairs = _moved("xyz")
        m0 = uc.model("salt")
        K, Cv = coulomb.debye(0.5, R_MIN, R_MAX, NKC, prefactor=3.0)
        nl.set_coulomb_table(K, Cv, R_MIN, R_MAX)
        chg = -0.5 * uc.charges("salt")
        chg[::3] *= 2.0
        nl._charges.copy_(_charge_tensor(nl, chg))
        m = uc.Model(m0.F, m0.U, R_MIN, R_MAX, K, Cv, R_MIN, R_MAX, chg)
        _check(*replay(), uc.coul_reference(q, box6, mask, m, pairs), np.float32)

    contract.captured(COUL, full, before, after)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces and 8 NaN totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat both are finite."""
    def set_tables(nl):  # (a uniform random box has close pairs: both tables start near 0)
        nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, R_MAX, NK), 1e-3, R_MAX)
        nl.set_coulomb_table(*coulomb.ewald_real(uc.ALPHA, 1e-3, R_MAX, NKC), 1e-3, R_MAX)
        nl.set_charges(_charge_tensor(nl, np.where(np.arange(20000) % 2 == 0, 1.0, -1.0)))

    contract.failed_list(COUL, set_tables, lambda nl, qd: None)  # (no scratch before the capacity shrinks)


@gpu
@pytest.mark.parametrize("off", [32, 64])
@pytest.mark.parametrize("full", [False, True])
def test_both_offset_widths(full, off):
    contract.both_offset_widths(COUL, full, off)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_distributed_lists_are_refused(full):
    contract.distributed_lists_are_refused(COUL, full)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_slab_lists_without_local_ids_are_refused(full):
    """A slab build made without nl_set_local_ids holds global ids: NL_ERR_STATE from all four calls, as nl_table_forces."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError
    from tests.test_slab_paths import slab_parts

    box, dtype, rc = "xyz", np.float32, 3.4
    box6, mask = LJ_BOXES[box]
    q = _input(box, False)
    part = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 2), (2, 4)), mask)[0]
    nl = _handle(box, dtype, full, rc)
    nl.Initialize(N)
    _set(nl, "salt", rc, order=part["order"])
    qd = _torch().from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
    nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"])
    for call in (nl.coul_forces, nl.coul_virial):
        for wait in (True, False):
            with pytest.raises(NLError) as e:
                call(qd, wait=wait)
            assert e.value.code == NL_ERR_STATE


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,drift", [("xyz", True), ("open", False)])
def test_local_index_slabs(box, drift, full, dtype):
    """3 slabs, one after the other on the one device, the ghosts' charges supplied in the order of the slab's rows: every
    owned particle's force within the bound of the whole-box reference, the ranks' 8 doubles add up to the whole-box totals
    within the bound, n_in exactly."""
    from tests.test_slab_paths import slab_parts

    torch = _torch()
    rc, kind = 3.4, "salt"
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    (want, S), (ww, SW) = uc.ref(box, drift, kind)
    parts = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 1), (1, 3), (3, 4)), mask)
    assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(N))
    nl = _handle(box, dtype, full, rc)
    nl.set_local_ids(True)
    nl.Initialize(N)
    tot = np.zeros(8)
    for part in parts:
        assert len(part["order"]) > len(part["own"])  # ghosts
        _set(nl, kind, rc, order=part["order"])
        qd = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
        nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"])
        f, w = nl.coul_forces(qd).cpu().numpy(), nl.coul_virial(qd).cpu().numpy()
        assert f.shape == (len(part["own"]), 4)
        check_lj(f, want[part["own"]], S[part["own"]], dtype, c=COUL_C)
        tot += w
    check_virial(tot, ww, SW, dtype, c=COUL_CW)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_after_resort(full):
    """The charges are permuted with nl_resort like the positions; after the rebuild the forces are those of the permuted
    input, and the totals those of the box."""
    box, drift, kind, dtype = "xyz", True, "typed3", np.float32
    nl, qd = _built(_input(box, drift), box, dtype, full, 2.5, kind)
    order = nl.cell_order().cpu().numpy().copy()
    assert not np.array_equal(order, np.arange(N)) and np.array_equal(np.sort(order), np.arange(N))
    chg = nl._charges
    nl.resort(qd, chg)
    assert np.array_equal(chg.cpu().numpy(), uc.charges(kind)[order].astype(dtype))
    nl.MakeNeighList(qd, N)
    (want, S), (ww, SW) = uc.ref(box, drift, kind)
    _check(nl.coul_forces(qd), nl.coul_virial(qd), ((want[order], S[order]), (ww, SW)), dtype)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    F, U, _, _ = _tab("morse")
    F3, U3, types, _ = _tab("typed3")
    K, Cv = uc.coul_tab()
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    cd = _charge_tensor(nl, uc.charges("salt"))
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    shim = _WithCharges(lib, cd)
    calls = contract.entry_calls(COUL, shim, fd, out)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    set_pair = lambda: nl.set_pair_table(F, U, R_MIN, R_MAX)  # noqa: E731
    set_coul = lambda: nl.set_coulomb_table(K, Cv, R_MIN, R_MAX)  # noqa: E731
    # neither table: the getter, the wrapper, and the calls after a build; then each table alone
    assert nl.coulomb_table_info() is None
    assert lib.nl_get_coulomb_table(nl._h, 0, None, None, None, None) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for tables in ((), (set_pair,), (nl.clear_pair_table, set_coul)):
        for t in tables:
            t()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    assert nl.coulomb_table_info() == dict(nknots=NKC, r_min=R_MIN, r_max=R_MAX, lds=False)  # (no pair table to stage with)
    set_pair()
    assert nl.coulomb_table_info()["lds"]
    # no charges: NULL is NL_ERR_ARG, through the wrapper too; charges of another type or length are the wrapper's errors
    for name, o in zip(ENTRY, (fd, fd, out, out)):
        assert getattr(lib, name)(nl._h, qd.data_ptr(), 4, None, o.data_ptr(), None) == NL_ERR_ARG
    for call in (nl.coul_forces, nl.coul_virial):
        with pytest.raises(NLError) as e:
            call(qd)
        assert e.value.code == NL_ERR_ARG
        with pytest.raises(TypeError):
            call(qd, charges=cd.double())
        with pytest.raises(ValueError):
            call(qd, charges=cd[:-1].contiguous())
    with pytest.raises(TypeError):
        nl.set_charges(cd.cpu())
    nl.set_charges(cd)
    want = nl.coul_virial(qd).cpu().numpy()  # (reproducible bit for bit; a half list's forces are not)
    assert np.array_equal(nl.coul_virial(qd, charges=cd.clone()).cpu().numpy(), want)
    # the setter's arguments: each refused, and the table that was set is kept
    bad_k, bad_c = K.copy(), Cv.copy()
    bad_k[7], bad_c[-1] = np.inf, np.nan
    big = np.zeros(4097)
    for args in ((0, NKC, R_MIN, R_MAX, dp(K), None), (0, NKC, R_MIN, R_MAX, None, dp(Cv)), (0, 1, R_MIN, R_MAX, dp(K), dp(Cv)),
                 (0, -3, R_MIN, R_MAX, dp(K), dp(Cv)), (0, 4097, R_MIN, R_MAX, dp(big), dp(big)), (0, NKC, 0.0, R_MAX, dp(K), dp(Cv)),
                 (0, NKC, -1.0, R_MAX, dp(K), dp(Cv)), (0, NKC, R_MAX, R_MAX, dp(K), dp(Cv)), (0, NKC, R_MIN, np.inf, dp(K), dp(Cv)),
                 (0, NKC, np.nan, R_MAX, dp(K), dp(Cv)), (0, NKC, R_MIN, R_MAX, dp(bad_k), dp(Cv)), (0, NKC, R_MIN, R_MAX, dp(K), dp(bad_c)),
                 (1, NKC, R_MIN, R_MAX, dp(K), dp(Cv)), (2, NKC, R_MIN, R_MAX, dp(K), dp(Cv)), (-1, NKC, R_MIN, R_MAX, dp(K), dp(Cv)),
                 (1, 0, R_MIN, R_MAX, None, None)):
        assert lib.nl_set_coulomb_table(nl._h, *args) == NL_ERR_ARG, args[:4]
        assert nl.coulomb_table_info() == dict(nknots=NKC, r_min=R_MIN, r_max=R_MAX, lds=True)
    assert lib.nl_set_coulomb_table(None, 0, NKC, R_MIN, R_MAX, dp(K), dp(Cv)) == NL_ERR_ARG
    for which in (1, 2, -1):
        assert lib.nl_get_coulomb_table(nl._h, which, None, None, None, None) == NL_ERR_ARG
    assert lib.nl_get_coulomb_table(None, 0, None, None, None, None) == NL_ERR_ARG
    assert nl.coul_virial(qd).cpu().numpy().tobytes() == want.tobytes() and np.isfinite(want).all()
    with pytest.raises(TypeError):
        nl.set_coulomb_table(K, Cv[:-1], R_MIN, R_MAX)
    with pytest.raises(TypeError):
        nl.set_coulomb_table(np.zeros((2, 8)), np.zeros((2, 8)), R_MIN, R_MAX)  # one slot: no rows
    for excluded_call in (lambda: nl.set_coulomb_table(K, Cv, R_MIN, R_MAX, excluded=True), lambda: nl.coulomb_table_info(excluded=True),
                          lambda: nl.clear_coulomb_table(excluded=True)):
        with pytest.raises(ValueError):
            excluded_call()
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_coul)

    # the reach of both tables, and of each alone: rc = 2.9, skin = 0.3
    def set_both(r_max):
        nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, r_max, NK), R_MIN, r_max)
        nl.set_coulomb_table(*uc.coul_tab(NKC, R_MIN, r_max), R_MIN, r_max)

    def set_charge_table_only(r_max):
        set_pair()
        nl.set_coulomb_table(*uc.coul_tab(NKC, R_MIN, r_max), R_MIN, r_max)

    def set_pair_table_only(r_max):
        nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, r_max, NK), R_MIN, r_max)
        set_coul()

    for set_r_max in (set_both, set_charge_table_only, set_pair_table_only):
        contract.reach(COUL, nl, qd, set_r_max)
    set_pair(), set_coul()
    contract.clearing(COUL, nl, qd, set_coul, lambda: lib.nl_set_coulomb_table(nl._h, 0, 0, R_MIN, R_MAX, dp(K), dp(Cv)))
    set_coul()
    # three types; and a charge table beyond the smallest rc_ab (2.55) while the pair table stays within it
    contract.several_types(COUL, nl, qd, types, set_pair, lambda: nl.set_pair_table(F3, U3, R_MIN, R_MAX))
    nl.set_coulomb_table(*uc.coul_tab(NKC, R_MIN, 2.6), R_MIN, 2.6)
    for call in (nl.coul_forces, nl.coul_virial):
        with pytest.raises(NLError) as e:
            call(qd)
        assert e.value.code == NL_ERR_ARG
    assert torch.isfinite(nl.table_virial(qd)).all()
    # a first call of the totals inside a capture, on a handle whose scratch does not exist yet
    fresh = _handle("open", np.float32, False, 2.9)
    fresh.Initialize(N)
    _set(fresh, "salt", 2.9)
    fresh.MakeNeighList(qd, N)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(NLError) as e:
            fresh.coul_virial(qd, wait=False)
        fresh.coul_forces(qd, wait=False, out=fd)
    assert e.value.code == NL_ERR_STATE
    contract.no_particles(COUL, shim, False, lambda empty: _set(empty, "salt", 2.9), qd, fd, out)

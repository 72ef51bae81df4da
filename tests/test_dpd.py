"""The DPD pair thermostat (nl_set_dpd, nl_dpd_forces, nl_dpd_virial and their enqueue variants) against an O(N^2) float64
evaluation of the rule of include/nl_hip.h, with an error bound per particle and per component; the pair noise against its
numpy mirror, integer by integer; and the samplers of md_neighbor_list_amd.dpd.

Contract tested (include/nl_hip.h, nl_set_dpd):
  * |got - want| <= DPD_C u S for every particle and each of fx, fy, fz, pe on its own, and <= DPD_CW u S for each of the 7
    sums of the totals, n_in exact: want the float64 sum of tests.util_dpd dpd_reference (pair_table.interpolate on the pair
    table, dpd.interpolate on the weight table, dpd.pair_noise; no list), S the uncancelled sums with the conditioning of both
    table reads on the rounding of r2 and of dot on the rounding of dv;
  * gamma = sigma = 0 gives nl_table_forces; after a full build the two particles of an isolated pair receive exactly opposite
    forces; the same step gives the same bits, another step or seed another force for every pair;
  * the 24-bit integer of every pair, recovered from the forces of isolated dimers, is dpd.pair_noise_int;
  * a pair below r_min of the weight table gives NaN to exactly its two particles and to all 8 totals;
  * the LDS and the global path compute the same bits; a captured step that advances the step word draws fresh noise at
    every replay; what tests.consumer_contract states for every table-driven consumer.

The constants are not fitted to the kernel.  DPD_C and DPD_CW are 4 x the largest |emulated - want| / (u S) that a numpy
emulation of the rule reaches (tests.util_dpd dpd_emulate: one rounding per operation, no FMA, every particle's terms summed
in a random order; dpd_virial_emulate: the kernels' own summation tree in both position types) over the boxes and orders of
util_coulomb.EMULATED, three summation orders each; test_emulation_gives_c recomputes both maxima.  The factor 4 covers the
GPU's other summation order within a row.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import dpd, pair_table, rdf
from tests import consumer_contract as contract
from tests import util_dpd as ud
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _handle, _off_the_band, _pair_tab, _tab, _tdt, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_unit
from tests.util_coulomb import EMULATED
from tests.util_dpd import DPD_C, DPD_CW, DT, EMULATED_MAX, EMULATED_MAX_W, KINDS, NKD, SEED, STEP
from tests.util_table import morse, table_reference
from tests.virial_util import check_virial, virial_ratio

RC_LISTS = (2.5, 3.4)
GRID = (R_MIN, R_MAX, NKD)
LDS_BYTES = 65280  # NL_TABLE_LDS_BYTES of include/nl_hip.h (test_lds_and_global_paths reads it there)
ENTRY = ("nl_dpd_forces", "nl_dpd_forces_enqueue", "nl_dpd_virial", "nl_dpd_virial_enqueue")
KIND_OF = {"salt": "one", "typed3": "typed3"}  # (the kinds of util_coulomb.EMULATED as this family's)


# ------------------------------------------------------------------------------------------------- CPU: the pair noise
def test_noise_known_answers_and_symmetry():
    """The three values the rule gives at seed 0, step 0; the integer is odd, below 2^24, symmetric in (i, j) and exact in
    float32; fp32 and fp64 hold the same number up to the rounding of the one constant."""
    xi = dpd.pair_noise([0, 0, 1], [1, 2, 2], 0, 0)
    assert np.allclose(xi, [-0.56060726, 1.24249172, 1.55310388], rtol=0, atol=5e-9), xi
    rng = np.random.default_rng(1)
    i, j = rng.integers(0, 2 ** 31 - 1, size=(2, 20000))
    for seed, step in ((SEED, 0), (2 ** 64 - 1, 2 ** 40 + 3), (0, 2 ** 64 - 1)):
        m = dpd.pair_noise_int(i, j, seed, step)
        assert m.dtype == np.int64 and np.all(m % 2 != 0) and np.abs(m).max() < 2 ** 24
        assert np.array_equal(m, dpd.pair_noise_int(j, i, seed, step))
        assert np.array_equal(m.astype(np.float32).astype(np.int64), m)
        x32, x64 = dpd.pair_noise(i, j, seed, step, np.float32), dpd.pair_noise(i, j, seed, step)
        assert x32.dtype == np.float32 and np.abs(x32 - x64).max() <= 2.0 ** -23 * np.sqrt(3.0)
    assert int(dpd.pair_key(0, 0)) == int(dpd.fin(dpd.fin(np.array([0], dtype=np.uint64)))[0])
    assert np.array_equal(dpd.pair_noise_int(3, 5, 9, 2 ** 64 + 4), dpd.pair_noise_int(3, 5, 9, 4))  # (modulo 2^64)


def test_noise_statistics():
    """All 3 763 396 pairs of n = 2744 at seed 12345, steps 0 and 1, and seed 12346: mean, variance, the correlation between
    steps, between seeds and between the horizontally adjacent pairs (i, j), (i, j + 1), each within 5 standard errors."""
    n = 2744
    i, j = np.triu_indices(n, 1)
    M = len(i)
    assert M == 3763396
    x0, x1, xs = dpd.pair_noise(i, j, 12345, 0), dpd.pair_noise(i, j, 12345, 1), dpd.pair_noise(i, j, 12346, 0)
    se = 1.0 / np.sqrt(M)
    got = {"mean": abs(x0.mean()) / se, "var": abs(x0.var() - 1.0) / np.sqrt(0.8 / M), "steps": abs(np.mean(x0 * x1)) / se,
           "seeds": abs(np.mean(x0 * xs)) / se}
    adj = np.flatnonzero(j[:-1] + 1 == j[1:])  # (i, j) and (i, j + 1) of one row
    assert np.array_equal(i[adj], i[adj + 1]) and len(adj) == M - (n - 1)
    got["adjacent"] = abs(np.mean(x0[adj] * x0[adj + 1])) * np.sqrt(len(adj))
    print({k: round(float(v), 2) for k, v in got.items()})
    assert all(v <= 5.0 for v in got.values()), got
    assert abs(np.abs(x0).max() - np.sqrt(3.0)) < 1e-4 and not np.array_equal(x0, x1)


# --------------------------------------------------------------------------------------------------- CPU: the samplers
def test_samplers():
    r = pair_table.knots(*GRID)
    for s in (1.0, 0.5, 2.0):
        A = dpd.weight(*GRID, s=s)
        assert A.shape == (NKD,) and A.dtype == np.float64 and A[-1] == 0.0 and np.all(A[:-1] > 0)
        assert np.allclose((A * r) ** 2, (1.0 - r / R_MAX) ** (2 * s), rtol=1e-13, atol=1e-15)  # A^2 r^2 = w^2
    a, inn = dpd.interpolate(dpd.weight(*GRID), R_MIN, R_MAX, np.array([0.0, 0.5 * R_MIN ** 2, R_MIN ** 2, R_MAX ** 2]))
    assert a[0] == 0.0 and np.isnan(a[1]) and a[2] == dpd.weight(*GRID)[0] and a[3] == 0.0 and list(inn) == [False, True, True, False]
    # conservative: F = -U'(r) / r by central differences of its own U (a table of two knots at r -+ h gives U there);
    # U is quadratic inside r_c: the central difference is exact up to rounding
    a_, rc, h = 25.0, 2.0, 1e-5
    F, U = dpd.conservative(a_, rc, *GRID)
    assert F.shape == U.shape == (NKD,) and np.all(F[r >= rc] == 0) and np.all(U[r >= rc] == 0) and U[0] > 1.0
    for k in range(0, NKD, 29):
        if abs(r[k] - rc) < 2 * h:
            continue
        (_, lo), (_, hi) = (dpd.conservative(a_, rc, r[k] + s * h, r[k] + s * h + 1.0, 2) for s in (-1.0, 1.0))
        assert abs(-(hi[0] - lo[0]) / (2 * h) / r[k] - F[k]) <= 1e-8 * (abs(F[k]) + 1.0), k
    g = np.array([4.5, 0.0, 2.0])
    assert np.allclose(dpd.sigma_for(g, 1.5) ** 2, 2 * g * 1.5, rtol=1e-15) and dpd.sigma_for(4.5, 1.0) == 3.0


# --------------------------------------------------------------------------------------------------- CPU: the checker
def test_inputs():
    v = ud.velocities()
    assert v.shape == (N, 3) and np.array_equal(v, v.astype(np.float32)) and 0.5 < v.std() < 1.5
    for kind in KINDS:
        m = ud.model(kind)
        assert m.A.shape == (NKD,) and NKD != NK and len(m.gamma) == rdf.nslots(m.nt)
    m = ud.model("typed3")
    assert m.nt == 3 and m.F.shape == (6, NK) and m.rc_ab[0, 2] == 0 and set(m.types.tolist()) == {0, 1, 2}
    assert m.sigma[rdf.slot(1, 1, 3)] == 0 < m.gamma[rdf.slot(1, 1, 3)] and m.gamma[rdf.slot(0, 1, 3)] == 0


def test_reference_properties():
    """dpd_reference conserves momentum (Newton's third law pair by pair), is Galilean invariant (a common velocity added to
    everybody changes nothing), reduces to the pair table's reference for gamma = sigma = 0, and its friction opposes
    the relative motion: sum_i f_i . v_i of the friction alone is negative."""
    box, drift = "tilt", True
    box6, mask = LJ_BOXES[box]
    q, pairs, v = _input(box, drift), _pairs(box, drift), ud.velocities()
    m = ud.model("typed3")
    (want, S), (w, SW) = ud.dpd_reference(q, v, box6, mask, m, STEP, pairs)
    assert np.abs(want[:, :3].sum(axis=0)).max() <= 1e-12 * S[:, :3].sum()
    (boost, _), _ = ud.dpd_reference(q, v + np.array([3.0, -1.0, 2.0]), box6, mask, m, STEP, pairs)
    assert np.abs(boost - want)[:, :3].max() <= 1e-12 * S[:, :3].max()
    zero = ud.Model(m.F, m.U, R_MIN, R_MAX, m.A, R_MIN, R_MAX, 0 * m.gamma, 0 * m.sigma, DT, SEED, m.types, m.rc_ab)
    assert np.array_equal(ud.dpd_reference(q, v, box6, mask, zero, STEP, pairs)[0][0],
                          table_reference(q, box6, mask, m.F, m.U, R_MIN, R_MAX, pairs, m.types, m.rc_ab)[0])
    Fz = np.zeros_like(m.F)
    fric = ud.Model(Fz, Fz, R_MIN, R_MAX, m.A, R_MIN, R_MAX, m.gamma, 0 * m.sigma, DT, SEED, m.types, m.rc_ab)
    (ff, _), _ = ud.dpd_reference(q, v, box6, mask, fric, STEP, pairs)
    assert (ff[:, :3] * v).sum() < -100.0
    (other, _), _ = ud.dpd_reference(q, v, box6, mask, m, STEP + 1, pairs)
    assert np.abs(other - want)[:, :3].max() > 1.0 and np.array_equal(other[:, 3], want[:, 3])  # another step: other noise, the same pe
    assert w[7] > 10 * N and abs(w[6] - want[:, 3].sum()) <= 1e-12 * SW[6]


def test_emulation_gives_c():
    """DPD_C and DPD_CW = 4 x the largest |emulated - want| / (u S) of a numpy emulation of the kernel's arithmetic (never
    the kernel) against the float64 reference: per particle and component in fp32, the totals in both position types."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    v = ud.velocities()
    for box, drift, ckind in EMULATED:
        kind = KIND_OF[ckind]
        box6, mask = LJ_BOXES[box]
        m = ud.model(kind)
        (want, S), (ww, SW) = ud.ref(box, drift, kind)
        I, J = ud.listed(m, *_pairs(box, drift)[:2])
        q = _input(box, drift)
        vals = {T: ud.dpd_emulate_pairs(q, v, box6, mask, m, STEP, T, (I, J)) for T in DTYPES}
        for order in range(3):
            rng = np.random.default_rng(100 + order)
            f = ud.dpd_emulate(q, v, box6, mask, m, STEP, np.float32, rng, (I, J))
            r = lj_ratio(f, want, S, np.float32).max(axis=0)
            rw = []
            for T in DTYPES:  # (the totals are summed in double whatever T is: in fp64 that sum is the error)
                w = ud.dpd_virial_emulate(N, I, vals[T], rng)
                assert w[7] == ww[7]
                rw.append(virial_ratio(w, ww, SW, T))
            print(box, drift, kind, order, r.round(2), rw[0].round(3), rw[1].round(3))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, np.maximum(*rw))
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX <= DPD_C / 4
    assert worst_w.max() <= EMULATED_MAX_W <= DPD_CW / 4
    assert EMULATED_MAX - worst.max() < 0.01 and EMULATED_MAX_W - worst_w.max() < 0.001  # the constants are the measured maxima


def test_wrong_results_are_rejected():
    """check_lj under the fp32 bound refuses every mistake of util_dpd.DEFECTS made in the emulator: an unsymmetrised key,
    step + 1, A for A A in the friction, sigma without 1 / sqrt(dt), the friction's sign, v_j - v_i, the wrong slot's
    parameters with three types, a half list's reaction without the DPD term.  The emulator without a defect passes."""
    v = ud.velocities()
    for box, drift, kind in (("xyz", False, "one"), ("tilt", True, "typed3")):
        box6, mask = LJ_BOXES[box]
        m = ud.model(kind)
        (want, S), _ = ud.ref(box, drift, kind)
        pairs = ud.listed(m, *_pairs(box, drift)[:2])
        q = _input(box, drift)
        rng = np.random.default_rng(5)
        check_lj(ud.dpd_emulate(q, v, box6, mask, m, STEP, np.float64, rng, pairs), want, S, np.float32, c=DPD_C)
        for defect in ud.DEFECTS:
            if defect == "wrong slot" and kind == "one":
                continue  # (one slot has no wrong one)
            with pytest.raises(AssertionError):
                check_lj(ud.dpd_emulate(q, v, box6, mask, m, STEP, np.float64, rng, pairs, defect), want, S, np.float32, c=DPD_C)


# ------------------------------------------------------------------------------------------------------ GPU helpers
class _WithDpd:
    """The library as tests.consumer_contract calls it -- fn(handle, q, stride, out, stream) -- with the velocities, their
    stride and the step word put in for the four entry points; every other call, and a call that brings its own, goes
    through unchanged."""

    def __init__(self, lib, v, step):
        self.__dict__.update(_lib=lib, _v=v, _step=step)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY:
            return fn
        return lambda *a: fn(*a) if len(a) == 8 else fn(*a[:3], self._v.data_ptr(), self._v.shape[1], self._step.data_ptr(), *a[3:])


def _dev(nl, values):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.float64))).to(nl.dtype).cuda()


def _step_word(step):
    return _torch().tensor([step], dtype=_torch().int64, device="cuda")


def _attach(nl, v, step=STEP):
    """The thin shim of the contract: nl.t_forces(q, wait, out) and nl.t_virial are dpd_forces and dpd_virial with the
    handle's velocities (the first len(q) rows: a slab's build has fewer) and step word, and nl._lib puts them into the C
    calls."""
    nl.t_v, nl.t_step = _dev(nl, v), _step_word(step)
    nl.t_forces = lambda q, wait=True, out=None: nl.dpd_forces(q, nl.t_v[:len(q)], nl.t_step, wait=wait, out=out)
    nl.t_virial = lambda q, wait=True, out=None: nl.dpd_virial(q, nl.t_v[:len(q)], nl.t_step, wait=wait, out=out)
    if not isinstance(nl._lib, _WithDpd):
        nl._lib = _WithDpd(nl._lib, nl.t_v, nl.t_step)


def _set(nl, kind, rc, nk=NK, nkd=NKD, vstride=3, seed=SEED):
    """The kind's pair table (and type table at the list's cut-off), the weight table and the parameters onto an initialised
    handle, and the shim with the velocities."""
    F, U, types, rc_ab = ud.pair_tab(kind, nk)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    nl.set_dpd(ud.weight_tab(nkd), *ud.params(kind), R_MIN, R_MAX, DT, seed)
    v = ud.velocities()
    _attach(nl, v if vstride == 3 else np.concatenate([v, np.full((N, 1), 77.0)], axis=1))


def _check(f, w, refs, dtype, rows=None):
    (want, S), (ww, SW) = refs
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, want, S, dtype).max(axis=0).round(2), virial_ratio(w, ww, SW, dtype).round(2))
    check_lj(f, want, S, dtype, c=DPD_C, rows=rows)
    if rows is None:
        check_virial(w, ww, SW, dtype, c=DPD_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (DPD_C + DPD_CW) * lj_unit(dtype) * SW[6]
    return f, w


DPD = contract.Consumer(
    forces="t_forces", virial="t_virial", scratch="t_virial", clear="clear_dpd", info="dpd_info", entry=ENTRY,
    set=_set, kinds=KINDS, ref=ud.ref, moved_ref=ud.moved_ref, extra=lambda nl: (),
    check=lambda f, w, x, refs, dtype, rows=None: _check(f, w, refs, dtype, rows), half_lists=True, local_slabs=False)
_built = functools.partial(contract.built, DPD)
gpu = pytest.mark.gpu


def _refs(q, box, m, pairs, step=STEP, v=None):
    box6, mask = LJ_BOXES[box]
    return ud.dpd_reference(q, ud.velocities() if v is None else v, box6, mask, m, step, pairs)


def _info(kind, lds, nkd=NKD):
    return dict(ntypes=ud.model(kind).nt, nknots=nkd, r_min=R_MIN, r_max=R_MAX, dt=DT, seed=SEED, lds=lds)


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x both kinds (one type; three types with a pair rc_ab = 0) x list kind x dtype; the
    list cut-off (2.5; 3.4, whose rows are longer than one wave trip), the offset width and the strides of q and v rotate
    through the cases.  Two calls of the totals are bit-identical."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, kind in enumerate(KINDS):
        k = case + p + (1 if full else 0)
        rc, off, stride = RC_LISTS[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        vstride = (3, 4)[(k // 2) % 2]
        nl, qd = _built(q, box, dtype, full, rc, kind, off, stride, vstride=vstride)
        assert nl.build_info()["offset_bits"] == off and qd.shape[1] == stride and nl.t_v.shape[1] == vstride
        knots = np.atleast_2d(ud.pair_tab(kind)[0]).size + NKD + rdf.nslots(ud.model(kind).nt)
        assert nl.dpd_info() == _info(kind, knots * 4 * np.dtype(dtype).itemsize <= LDS_BYTES)  # (typed3: 6 slots, global)
        f, w = nl.t_forces(qd), nl.t_virial(qd)
        assert f.shape == (N, 4) and f.dtype == _tdt(dtype) and w.shape == (8,) and w.dtype == _torch().float64
        _, w = _check(f, w, ud.ref(box, drift, kind), dtype)
        assert w.tobytes() == nl.t_virial(qd).cpu().numpy().tobytes() and len(w.tobytes()) == 64


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "typed3"), ("xyz", False, "one")])
def test_no_friction_and_no_noise_are_the_pair_table(box, drift, kind, dtype):
    """A full list, gamma = sigma = 0: forces, energies and the 7 sums equal nl_table_forces' and nl_table_virial's by value
    (== and not bits: the sign of a zero may differ), n_in as well; a Python int serves as the step of a blocking call."""
    nl, qd = _built(_input(box, drift), box, dtype, True, 3.4, kind)
    g, _ = ud.params(kind)
    nl.set_dpd(ud.weight_tab(), 0 * g, 0 * g, R_MIN, R_MAX, DT, SEED)
    f, w = nl.dpd_forces(qd, nl.t_v, 5).cpu().numpy(), nl.dpd_virial(qd, nl.t_v, 2 ** 64 - 1).cpu().numpy()
    ft, wt = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert np.isfinite(ft).all() and np.abs(ft).max() > 0.1 and wt[7] > 10 * N
    assert np.all(f == ft) and np.all(w == wt)
    with pytest.raises(TypeError):
        nl.dpd_forces(qd, nl.t_v, 5, wait=False)  # (the enqueue variants copy nothing from the host)


def _dimer_cloud(m_dimers, seed=3, grid=2.0 ** -20):
    """m isolated two-particle molecules in an open box, rows shuffled: centres on a grid of spacing 2.5, separations of
    length 0.4 to 0.8, coordinates multiples of `grid` (2^-20: exact in float64; 2^-16: in float32 too, below 128), so that
    the separations are exact in the position type.  Returns (q[2 m, 3], box, a[m], b[m]: the rows of each dimer's two
    particles)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(m_dimers ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:m_dimers]
    mid = (g + 0.5) * 2.5
    u = rng.normal(size=(m_dimers, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = rng.uniform(0.4, 0.8, size=m_dimers)
    p1 = np.round((mid - 0.5 * r[:, None] * u) / grid) * grid
    p2 = np.round((mid + 0.5 * r[:, None] * u) / grid) * grid
    perm = rng.permutation(2 * m_dimers)
    q = np.empty((2 * m_dimers, 3))
    q[perm[:m_dimers]], q[perm[m_dimers:]] = p1, p2
    return q, (side * 2.5,) * 3, perm[:m_dimers], perm[m_dimers:]


def _dimer_handle(q, box, dtype, full, rc=1.0):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box, dtype=_tdt(dtype), full_list=full, minimum_image=False)
    nl.Initialize(len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q.astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    assert nl.half_number_of_pairs() == len(q) // 2  # (every dimer, and nothing else)
    return nl, qd


@gpu
def test_the_integer_of_every_pair():
    """fp64, 33 000 isolated dimers in shuffled rows (ids above 2^16), phi = 0, gamma = 0, a step above 2^32: the integer
    2 m + 1 - 2^24 recovered from fx / (dx sg A) of each dimer is dpd.pair_noise_int of its two rows.  The reference is per
    dimer.  The recovered value is within 1e-6 of an integer: A is the double interpolation of exact separations."""
    md, seed, step, sigma, dt = 33000, 2 ** 63 + 12345, 2 ** 32 + 17, 3.0, 0.04
    q, box, a, b = _dimer_cloud(md)
    assert len(q) == 66000 and max(a.max(), b.max()) > 2 ** 16
    nl, qd = _dimer_handle(q, box, np.float64, True)
    r_min, r_max, nk = 0.3, 1.0, 256
    z = np.zeros(nk)
    A = dpd.weight(r_min, r_max, nk)
    nl.set_pair_table(z, z, r_min, r_max)
    nl.set_dpd(A, 0.0, sigma, r_min, r_max, dt, seed)
    assert nl.dpd_info()["seed"] == seed and nl.dpd_info()["lds"]
    vd = _torch().zeros((len(q), 3), dtype=_torch().float64, device="cuda")
    f = nl.dpd_forces(qd, vd, step).cpu().numpy()
    d = q[a] - q[b]
    av, inn = dpd.interpolate(A, r_min, r_max, (d * d).sum(axis=1))
    assert inn.all() and np.isfinite(av).all() and np.abs(d[:, 0]).min() > 0
    got = f[a, 0] / (d[:, 0] * (sigma / np.sqrt(dt)) * av) / dpd.XI_SCALE
    want = dpd.pair_noise_int(a, b, seed, step)
    assert np.abs(got - np.rint(got)).max() < 1e-6 and np.array_equal(np.rint(got).astype(np.int64), want)
    assert np.array_equal(f[a, :3], -f[b, :3]) and np.all(f[:, 3] == 0)
    assert not np.array_equal(want, dpd.pair_noise_int(a, b, seed, step - 2 ** 32))  # (the high word of the step counts)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_dimers_are_antisymmetric_reproducible_and_follow_step_and_seed(dtype):
    """A full list over 500 isolated dimers with a Morse pair table, friction and noise: f[i] == -f[j] bit for bit; the same
    step twice gives the same bits; another step, or another seed, changes the force of every dimer; a half list agrees with
    the float64 rule per dimer."""
    torch = _torch()
    q, box, a, b = _dimer_cloud(500, seed=8, grid=2.0 ** -16)
    assert np.array_equal(q, q.astype(np.float32))
    r_min, r_max, nk = 0.3, 1.0, 256
    F, U = pair_table.sample(*morse(r0=0.6), r_min, r_max, nk)
    A, g, s = dpd.weight(r_min, r_max, nk), 4.5, 3.0
    v = np.random.default_rng(2).normal(size=q.shape).astype(np.float32).astype(np.float64)
    d = q[a] - q[b]
    r2 = (d * d).sum(axis=1)
    for full in (True, False):
        nl, qd = _dimer_handle(q, box, dtype, full)
        nl.set_pair_table(F, U, r_min, r_max)
        nl.set_dpd(A, g, s, r_min, r_max, DT, SEED)
        vd, sw = torch.from_numpy(v.astype(dtype)).cuda(), _step_word(40)
        f = nl.dpd_forces(qd, vd, sw).cpu().numpy()
        fr = (pair_table.interpolate(F, U, r_min, r_max, r2)[0] - g * dpd.interpolate(A, r_min, r_max, r2)[0] ** 2 * (d * (v[a] - v[b])).sum(axis=1)
              + s / np.sqrt(DT) * dpd.interpolate(A, r_min, r_max, r2)[0] * dpd.pair_noise(a, b, SEED, 40))
        tol = (1e-5 if dtype == np.float32 else 1e-13) * (np.abs(fr) + 30.0)[:, None] * np.abs(d)
        assert np.all(np.abs(f[a, :3] - fr[:, None] * d) <= tol)
        assert np.array_equal(f[a, :3], -f[b, :3]) and np.array_equal(f[a, 3], f[b, 3])  # (one pair a particle: no sum to reorder)
        if not full:
            continue
        assert f.tobytes() == nl.dpd_forces(qd, vd, sw).cpu().numpy().tobytes()
        sw += 1
        f1 = nl.dpd_forces(qd, vd, sw).cpu().numpy()
        assert np.all((f1[a, :3] != f[a, :3]).any(axis=1)) and np.array_equal(f1[:, 3], f[:, 3])
        sw -= 1
        nl.set_dpd(A, g, s, r_min, r_max, DT, SEED + 1)
        f2 = nl.dpd_forces(qd, vd, sw).cpu().numpy()
        assert np.all((f2[a, :3] != f[a, :3]).any(axis=1))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,kind", [("tilt", True, "typed3"), ("xyz", False, "one")])
def test_half_and_full_agree(box, drift, kind, dtype):
    refs = ud.ref(box, drift, kind)
    got = {}
    for full in (False, True):
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, kind)
        got[full] = _check(nl.t_forces(qd), nl.t_virial(qd), refs, dtype)
    u = lj_unit(dtype)
    assert np.all(np.abs(got[False][0].astype(np.float64) - got[True][0]) <= 2 * DPD_C * u * refs[0][1])
    assert np.all(np.abs(got[False][1][:7] - got[True][1][:7]) <= 2 * DPD_CW * u * refs[1][1])
    assert got[False][1][7] == got[True][1][7] == refs[1][0][7]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,nk", [("one", NK), ("typed3", 128)])
def test_lds_and_global_paths(kind, nk, dtype, monkeypatch):
    """A DPD state set under NL_TABLE_LDS=0 makes the calls read all three tables from global memory.  On one list the two
    paths give the same bits: full-list forces and the totals of both list kinds; half-list forces within the bound.  Tables
    that do not fit NL_TABLE_LDS_BYTES together take the global path by themselves."""
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    lds_bytes = int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1))
    knot = 4 * np.dtype(dtype).itemsize
    assert lds_bytes == LDS_BYTES and (np.atleast_2d(ud.pair_tab(kind, nk)[0]).size + NKD + 6) * knot <= lds_bytes  # staged unless switched off
    box, drift = "tilt", True
    refs = _refs(_input(box, drift), box, ud.model(kind, nk), _pairs(box, drift))
    for full in (False, True):
        monkeypatch.delenv("NL_TABLE_LDS", raising=False)
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, kind, nk=nk)
        assert nl.dpd_info()["lds"]
        lds = _check(nl.t_forces(qd), nl.t_virial(qd), refs, dtype)
        monkeypatch.setenv("NL_TABLE_LDS", "0")
        nl.set_dpd(ud.weight_tab(), *ud.params(kind), R_MIN, R_MAX, DT, SEED)  # (the same state, the same list: the other path)
        assert not nl.dpd_info()["lds"]
        glo = _check(nl.t_forces(qd), nl.t_virial(qd), refs, dtype)
        assert lds[1].tobytes() == glo[1].tobytes() and len(glo[1].tobytes()) == 64
        if full:
            assert lds[0].tobytes() == glo[0].tobytes()
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nkd = 3584  # with the 1024 knots of the pair table: 4608 knots, 72 KiB in fp32 -- beyond LDS together, each within it alone
    assert (NK + nkd) * knot > lds_bytes
    big = ud.model("one", NK, nkd)
    nl, qd = _built(_input(box, drift), box, dtype, True, 3.4, "one", nkd=nkd)
    assert not nl.dpd_info()["lds"]
    _check(nl.t_forces(qd), nl.t_virial(qd), _refs(_input(box, drift), box, big, _pairs(box, drift)), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_a_pair_below_the_weight_table(full, dtype):
    """One particle moved to 0.5 from its neighbour, inside a pair table that starts at 0.4 and below r_min = 0.85 of the
    weight table, gamma = sigma = 0: NaN in exactly those two particles' forces and energies, 8 NaN totals, everybody else
    within the bound."""
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
    F, U = _pair_tab(1, 0.4, R_MAX, NK)
    m = ud.Model(F, U, 0.4, R_MAX, ud.weight_tab(), R_MIN, R_MAX, 0.0, 0.0)
    refs = _refs(q, box, m, pairs)
    nans = np.isnan(refs[0][0]).all(axis=1)
    assert np.array_equal(np.flatnonzero(nans), sorted((a, b))) and np.isnan(refs[1][0]).all()
    nl, qd = _built(q, box, dtype, full, 2.5, "one")
    nl.set_pair_table(F, U, 0.4, R_MAX)
    nl.set_dpd(ud.weight_tab(), 0.0, 0.0, R_MIN, R_MAX, DT, SEED)
    assert _torch().isfinite(nl.table_forces(qd)).all()  # (the pair table has a value there)
    f, w = nl.t_forces(qd).cpu().numpy(), nl.t_virial(qd).cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,)
    assert np.array_equal(np.isnan(f), np.repeat(nans[:, None], 4, axis=1))
    check_lj(f, *refs[0], dtype, c=DPD_C, rows=~nans)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,kind", [("xyz", "one"), ("tilt", "typed3")])
def test_reuse_within_the_skin(box, kind, full, dtype):
    contract.reuse_within_the_skin(DPD, box, kind, full, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """One graph holds the copy of the positions, nl_update_list, step += 1 on the device word, the forces and the totals.
    Three replays match the reference at the steps s + 1, s + 2, s + 3 (the second and third at moved positions, within the
    skin); then gamma, sigma, dt and the seed are changed through nl_set_dpd in place, and the fourth replay computes with them."""
    torch = _torch()
    dtype, box, kind, s0 = np.float32, "xyz", "one", 2 ** 33
    box6, mask = LJ_BOXES[box]
    q0, (q1, pairs1) = _input(box, False), _moved(box)
    nl = _handle(box, dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    _set(nl, kind, 2.9)
    nl.t_step.fill_(s0)
    src = torch.from_numpy(q0.astype(dtype)).cuda()
    qd = src.clone()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    nl.update(qd, sync=True)
    nl.update(qd)
    nl.t_virial(qd, wait=False, out=wd)  # once before the capture: the scratch exists
    nl.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        nl.t_step += 1
        nl.t_forces(qd, wait=False, out=fd)
        nl.t_virial(qd, wait=False, out=wd)
    m = ud.model(kind)
    for k, (q, pairs) in enumerate(((q0, _pairs(box, False)), (q1, pairs1), (q1, pairs1)), start=1):
        src.copy_(torch.from_numpy(q.astype(dtype)))
        fd.fill_(-1.0), wd.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert int(nl.t_step.item()) == s0 + k
        _check(fd, wd, _refs(q, box, m, pairs, step=s0 + k), dtype)
    g2, s2 = np.array([2.0]), np.array([1.0])
    nl.set_dpd(ud.weight_tab(), g2, s2, R_MIN, R_MAX, 0.04, SEED + 9)
    m2 = ud.Model(m.F, m.U, R_MIN, R_MAX, m.A, R_MIN, R_MAX, g2, s2, 0.04, SEED + 9)
    fd.fill_(-1.0), wd.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    _check(fd, wd, _refs(q1, box, m2, pairs1, step=s0 + 4), dtype)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces and 8 NaN totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat both are finite."""
    def set_tables(nl):  # (a uniform random box has close pairs: both tables start near 0)
        nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, R_MAX, NK), 1e-3, R_MAX)
        nl.set_dpd(dpd.weight(1e-3, R_MAX, NKD), 4.5, 3.0, 1e-3, R_MAX, DT, SEED)
        _attach(nl, ud.velocities(20000, seed=4))

    contract.failed_list(DPD, set_tables, lambda nl, qd: None)  # (no scratch before the capacity shrinks)


@gpu
@pytest.mark.parametrize("off", [32, 64])
@pytest.mark.parametrize("full", [False, True])
def test_both_offset_widths(full, off):
    contract.both_offset_widths(DPD, full, off)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_distributed_lists_are_refused(full):
    """A list of caller ids (a distributed build of a world of one): NL_ERR_STATE from all four calls."""
    contract.distributed_lists_are_refused(DPD, full)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_slab_lists_are_refused(full):
    """A slab build, with and without nl_set_local_ids: NL_ERR_STATE -- the noise is keyed by rows, and the two ranks of a
    crossing pair would key it differently."""
    contract.slab_lists_are_refused(DPD, full)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_after_resort(full):
    """Positions and velocities are permuted with nl_resort alike; after the rebuild the forces are those of the reference on
    the permuted arrays (the noise follows the new rows), and the totals are within the bound of that reference's."""
    box, drift, kind, dtype = "xyz", True, "typed3", np.float32
    box6, mask = LJ_BOXES[box]
    nl, qd = _built(_input(box, drift), box, dtype, full, 2.5, kind)
    order = nl.cell_order().cpu().numpy().copy()
    assert not np.array_equal(order, np.arange(N)) and np.array_equal(np.sort(order), np.arange(N))
    nl.resort(qd, nl.t_v)
    assert np.array_equal(nl.t_v.cpu().numpy(), ud.velocities()[order].astype(dtype))
    nl.MakeNeighList(qd, N)
    m = ud.model(kind)
    mp = ud.Model(m.F, m.U, R_MIN, R_MAX, m.A, R_MIN, R_MAX, m.gamma, m.sigma, DT, SEED, m.types[order], m.rc_ab)
    qp = _input(box, drift)[order]
    refs = ud.dpd_reference(qp, ud.velocities()[order], box6, mask, mp, STEP, lj_pairs(qp, box6, mask, R_MAX * (1 + 2.0 ** -16)))
    _check(nl.t_forces(qd), nl.t_virial(qd), refs, dtype)
    old = ud.ref(box, drift, kind)[0][0][order]
    assert np.abs(refs[0][0] - old)[:, :3].max() > 1.0  # (another noise for the physical pairs)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_on_a_callers_held_stream(dtype):
    """A non-blocking stream of the caller's, held back by a delay: the positions, the velocities and the step word are
    written behind the delay, and the update, the forces and the totals enqueued on that stream read what was written."""
    from tests.stream_util import device, held_stream, rolled

    torch = _torch()
    box, kind, full = "xyz", "one", True
    q, v = _input(box, False), ud.velocities()
    nl = _handle(box, dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    _set(nl, kind, 2.9)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    vsrc, ssrc = device(v, dtype), _step_word(STEP)
    qd = dec.clone()
    nl.t_v.copy_(device(rolled(v), dtype))
    nl.t_step.fill_(STEP + 5)
    fd = torch.empty((N, 4), dtype=_tdt(dtype), device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    nl.update(qd, sync=True)  # (warm, on the decoy: nothing allocates while the stream is held)
    nl.t_forces(qd, wait=False, out=fd), nl.t_virial(qd, wait=False, out=wd)
    torch.cuda.synchronize()
    with held_stream() as h:
        h.copy(qd, src), h.copy(nl.t_v, vsrc), h.copy(nl.t_step, ssrc)
        h.assert_held()
        nl.update(qd)
        nl.t_forces(qd, wait=False, out=fd), nl.t_virial(qd, wait=False, out=wd)
        h.assert_held(f"dpd {np.dtype(dtype).name}")
    nl.synchronize()
    _check(fd, wd, ud.ref(box, False, kind), dtype)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    F, U, _, _ = _tab("morse")
    F3, U3, types, _ = _tab("typed3")
    A = ud.weight_tab()
    g1, s1 = ud.params("one")
    g3, s3 = ud.params("typed3")
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    _attach(nl, ud.velocities())
    shim, vd, sw = nl._lib, nl.t_v, nl.t_step
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    calls = contract.entry_calls(DPD, shim, fd, out)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    set_pair = lambda: nl.set_pair_table(F, U, R_MIN, R_MAX)  # noqa: E731
    set_dpd = lambda: nl.set_dpd(A, g1, s1, R_MIN, R_MAX, DT, SEED)  # noqa: E731
    # neither table: the getter, the wrapper, and the calls after a build; then each alone
    assert nl.dpd_info() is None
    assert lib.nl_get_dpd(nl._h, None, None, None, None, None, None, None) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for tables in ((), (set_pair,), (nl.clear_pair_table, set_dpd)):
        for t in tables:
            t()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    assert nl.dpd_info() == _info("one", False)  # (no pair table to stage with)
    set_pair()
    assert nl.dpd_info() == _info("one", True)
    # the velocities and the step word: NULL is NL_ERR_ARG, as is a stride other than 3 or 4; the wrapper's own errors
    for name, o in zip(ENTRY, (fd, fd, out, out)):
        fn = getattr(lib, name)
        assert fn(nl._h, qd.data_ptr(), 4, None, 3, sw.data_ptr(), o.data_ptr(), None) == NL_ERR_ARG
        assert fn(nl._h, qd.data_ptr(), 4, vd.data_ptr(), 3, None, o.data_ptr(), None) == NL_ERR_ARG
        for stride in (0, 2, 5):
            assert fn(nl._h, qd.data_ptr(), 4, vd.data_ptr(), stride, sw.data_ptr(), o.data_ptr(), None) == NL_ERR_ARG
        assert fn(nl._h, qd.data_ptr(), 4, vd.data_ptr(), 3, sw.data_ptr(), o.data_ptr(), None) == 0
    for call in (nl.dpd_forces, nl.dpd_virial):
        for v_, s_ in ((None, sw), (vd, None)):
            with pytest.raises(NLError) as e:
                call(qd, v_, s_)
            assert e.value.code == NL_ERR_ARG
        with pytest.raises(TypeError):
            call(qd, vd.double(), sw)
        with pytest.raises(ValueError):
            call(qd, vd[:-1].contiguous(), sw)
        with pytest.raises(TypeError):
            call(qd, vd, sw.int())
    want = nl.t_virial(qd).cpu().numpy()  # (reproducible bit for bit; a half list's forces are not)
    assert np.array_equal(nl.dpd_virial(qd, vd.clone(), STEP).cpu().numpy(), want) and np.isfinite(want).all()
    # the setter's arguments: each refused, and the state that was set is kept
    bad_a, bad_g, neg_g, neg_s, inf_s = A.copy(), g1.copy(), g1.copy(), s1.copy(), s1.copy()
    bad_a[7], bad_g[0], neg_g[0], neg_s[0], inf_s[0] = np.inf, np.nan, -1.0, -0.5, np.inf
    big = np.zeros(4097)
    ok = (1, NKD, R_MIN, R_MAX, dp(A), dp(g1), dp(s1), DT, SEED)

    def but(**kw):
        names = ("ntypes", "nknots", "r_min", "r_max", "A", "gamma", "sigma", "dt", "seed")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for args in (but(A=None), but(gamma=None), but(sigma=None), but(A=None, gamma=None), but(nknots=1), but(nknots=-3),
                 but(nknots=4097, A=dp(big)), but(r_min=0.0), but(r_min=-1.0), but(r_min=R_MAX), but(r_max=np.inf), but(r_min=np.nan),
                 but(A=dp(bad_a)), but(gamma=dp(bad_g)), but(gamma=dp(neg_g)), but(sigma=dp(neg_s)), but(sigma=dp(inf_s)), but(ntypes=0),
                 but(ntypes=33), but(dt=0.0), but(dt=-0.01), but(dt=np.inf), but(dt=np.nan)):
        assert lib.nl_set_dpd(nl._h, *args) == NL_ERR_ARG, args[:4]
        assert nl.dpd_info() == _info("one", True)
    assert lib.nl_set_dpd(None, *ok) == NL_ERR_ARG and lib.nl_get_dpd(None, None, None, None, None, None, None, None) == NL_ERR_ARG
    assert nl.t_virial(qd).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(TypeError):
        nl.set_dpd(np.zeros((2, 8)), g1, s1, R_MIN, R_MAX, DT)  # one slot: no rows
    with pytest.raises(TypeError):
        nl.set_dpd(A, g3, s1, R_MIN, R_MAX, DT)
    with pytest.raises(TypeError):
        nl.set_dpd(A, g3[:4], s3[:4], R_MIN, R_MAX, DT)  # 4 slots are no ntypes (ntypes + 1) / 2
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_dpd)

    # the reach of both tables, and of each alone: rc = 2.9, skin = 0.3
    def set_both(r_max):
        nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, r_max, NK), R_MIN, r_max)
        nl.set_dpd(dpd.weight(R_MIN, r_max, NKD), g1, s1, R_MIN, r_max, DT, SEED)

    def set_weight_table_only(r_max):
        set_pair()
        nl.set_dpd(dpd.weight(R_MIN, r_max, NKD), g1, s1, R_MIN, r_max, DT, SEED)

    def set_pair_table_only(r_max):
        nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, r_max, NK), R_MIN, r_max)
        set_dpd()

    for set_r_max in (set_both, set_weight_table_only, set_pair_table_only):
        contract.reach(DPD, nl, qd, set_r_max)
    set_pair(), set_dpd()
    contract.clearing(DPD, nl, qd, set_dpd, lambda: lib.nl_set_dpd(nl._h, *but(nknots=0)))
    set_dpd()
    # three types of the pair table under one type of parameters; then three types of parameters under either pair table
    contract.several_types(DPD, nl, qd, types, set_pair, lambda: nl.set_pair_table(F3, U3, R_MIN, R_MAX))
    nl.set_dpd(A, g3, s3, R_MIN, R_MAX, DT, SEED)
    assert nl.dpd_info()["ntypes"] == 3 and torch.isfinite(nl.t_virial(qd)).all()
    set_pair()  # (a pair table of one type under parameters of three)
    assert torch.isfinite(nl.t_forces(qd)).all()
    nl.set_type_cutoffs(types % 2, [[2.9, 2.9], [2.9, 2.9]])
    nl.MakeNeighList(qd, N)
    with pytest.raises(NLError) as e:
        nl.t_forces(qd)
    assert e.value.code == NL_ERR_ARG  # parameters of 3 types against the type table's 2
    nl.clear_type_cutoffs()
    nl.MakeNeighList(qd, N)
    with pytest.raises(NLError) as e:
        nl.t_virial(qd)
    assert e.value.code == NL_ERR_STATE  # ... and against none
    set_dpd()
    # a weight table beyond the list's reach while the pair table stays within it
    nl.set_dpd(dpd.weight(R_MIN, 3.0, NKD), g1, s1, R_MIN, 3.0, DT, SEED)
    for call in (nl.t_forces, nl.t_virial):
        with pytest.raises(NLError) as e:
            call(qd)
        assert e.value.code == NL_ERR_ARG
    assert torch.isfinite(nl.table_virial(qd)).all()
    # a first call of the totals inside a capture, on a handle whose scratch does not exist yet
    fresh = _handle("open", np.float32, False, 2.9)
    fresh.Initialize(N)
    _set(fresh, "one", 2.9)
    fresh.MakeNeighList(qd, N)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(NLError) as e:
            fresh.t_virial(qd, wait=False)
        fresh.t_forces(qd, wait=False, out=fd)
    assert e.value.code == NL_ERR_STATE
    contract.no_particles(DPD, shim, False, lambda empty: _set(empty, "one", 2.9), qd, fd, out)

"""Tabulated pair potentials (nl_set_pair_table, nl_table_forces, nl_table_virial and their enqueue variants) against an
O(N^2) float64 sum of the interpolation rule, with an error bound per particle and per component.

Contract tested (include/nl_hip.h, nl_set_pair_table):
  * |got - want| <= TABLE_C u S for every particle and each of fx, fy, fz, pe on its own, and <= TABLE_CW u S for each of the
    7 sums of the totals, n_in exact: want the float64 sum of tests.util_table table_reference over pair_table.interpolate on
    the caller's double tables (no list, the library's or the oracle's), S the uncancelled sum of the pair terms
    (|F_k| + |F_k+1| + |dF_k| r2 / D) |d_c| -- the third term is the conditioning of s = (r2 - x0) / D on the rounding of r2;
  * a pair below r_min gives NaN to exactly its two particles and to all 8 totals;
  * the LDS and the global path compute the same bits.

The constants are not fitted to the kernel.  TABLE_C = 10.7 is 4 x the largest |emulated - want| / (u S) = 2.67 that a float32
numpy emulation of the rule reaches (tests.util_table table_emulate: one rounding per operation, no FMA, every particle's
terms summed in a random order, the knots and scalars rounded as the setter rounds them) over the inputs of EMULATED, three
summation orders each.  TABLE_CW = 1.95 is 4 x the 0.487 of the totals, which are emulated in both position types with the
kernels' own summation tree (tests.util_table table_virial_emulate): they are summed in double whatever T is, so in fp64 that
sum is the whole error and u S only a few ulp of the result (the fp32 emulation alone gives 0.197, and the kernel reached 0.9
on an fp64 list in its first run); for the same reason the totals' reference is summed in long double.
test_emulation_gives_c recomputes both maxima against the float64 reference.  The factor 4 covers the GPU's other summation
order within a row.

The inputs (tests.util lj_lattice, cuts = (R_MIN, R_MAX)): the 14^3 jittered lattice, n = 2744 > 4 NL_TABLE_BLOCKS rows, so
some waves of the persistent grid walk a second row; no pair within 2^-17 (relative, r^2) of r_max or r_min.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import pair_table, rdf
from tests import consumer_contract as contract
from tests.consumer_util import CASES, DTYPES, N, NK, R_MAX, R_MIN, _handle, _off_the_band, _tab, _tdt, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_C, LJ_M, ROOT, check_lj, lj_pairs, lj_ratio, lj_reference, lj_type_params, lj_unit
from tests.util_table import (TABLE_C, TABLE_CW, lj, lj_f_xx, lj_u_xx, morse, table_emulate, table_emulate_pairs, table_pairs,
                              table_reference, table_virial_emulate, table_virial_reference)
from tests.virial_util import check_virial, virial_ratio

NBLK = 512  # NL_TABLE_BLOCKS of include/nl_hip.h
RC_LISTS = (2.5, 3.4)
TABS = ("morse", "lj", "typed3")
# what the emulation that fixes TABLE_C and TABLE_CW runs over
EMULATED = [("open", False, "morse"), ("open", False, "lj"), ("xyz", False, "morse"), ("xyz", True, "lj"), ("tilt", False, "lj"),
            ("tilt", True, "morse"), ("xyz", True, "typed3"), ("tilt", True, "typed3")]
EMULATED_MAX, EMULATED_MAX_W = 2.67, 0.487  # the largest ratios of test_emulation_gives_c: per particle, and of the totals


# ------------------------------------------------------------------------------------------------ inputs, references
def _refs(q, box, tab, pairs, nk=NK):
    box6, mask = LJ_BOXES[box]
    F, U, types, rc_ab = _tab(tab, nk)
    kw = dict(pairs=pairs, types=types, rc_ab=None if rc_ab is None else rc_ab(3.4))
    return table_reference(q, box6, mask, F, U, R_MIN, R_MAX, **kw), table_virial_reference(q, box6, mask, F, U, R_MIN, R_MAX, **kw)


@functools.lru_cache(maxsize=None)
def _ref(box, drift, tab):
    """((want[n, 4], S[n, 4]), (want[8], S[7])) of an input and a table."""
    return _refs(_input(box, drift), box, tab, _pairs(box, drift))


@functools.lru_cache(maxsize=None)
def _moved_ref(box, tab, seed=21):
    q, pairs = _moved(box, seed)
    return _refs(q, box, tab, pairs)


def _single(tab):
    """(|F(r_max)| r_max, |U(r_max)| / 2) of the weakest slot of a table: the least a pair at r_max gives a particle."""
    F, U, _, _ = _tab(tab)
    F, U = np.atleast_2d(F), np.atleast_2d(U)
    live = np.abs(F).sum(axis=1) > 0
    return (np.abs(F[live, -1]) * R_MAX).min(), (0.5 * np.abs(U[live, -1])).min()


def _assert_sharp(refs, tab):
    (_, S), (_, SW) = refs
    Fm, Um = _single(tab)
    u = lj_unit(np.float32)
    assert np.all(TABLE_C * u * S[:, :3].max(axis=1) <= 0.25 * Fm / np.sqrt(3.0)), (TABLE_C * u * S[:, :3].max() / Fm)
    assert np.all(TABLE_C * u * S[:, 3] <= 0.25 * Um), (TABLE_C * u * S[:, 3].max() / Um)


# ------------------------------------------------------------------------------------------------- CPU: the checker
def test_header_states_the_constants():
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    assert int(re.search(r"#define NL_TABLE_BLOCKS\s+(\d+)", text).group(1)) == NBLK
    assert int(re.search(r"#define NL_TABLE_MAX_KNOTS\s+(\d+)", text).group(1)) == 4096
    assert N == 2744 > 4 * NBLK  # some waves of the persistent grid walk a second row, the last turn is ragged


def test_inputs():
    for box, drift in CASES:
        q = _input(box, drift)
        assert len(q) == N and np.array_equal(q[:, :3], q[:, :3].astype(np.float32))
        I, J, d, _ = _pairs(box, drift)  # (asserts the band)
        r = np.sqrt((d * d).sum(axis=1))
        assert R_MIN < 0.92 < r.min() < 0.95
    for tab in TABS:
        F, U, types, _ = _tab(tab)
        assert np.isfinite(F).all() and np.isfinite(U).all()
        Fm, Um = _single(tab)
        assert Fm > 0.03 and Um > 0.008  # the potentials do not vanish at r_max
    F, U, types, rc_ab = _tab("typed3")
    assert F.shape == (6, NK) and set(types.tolist()) == {0, 1, 2} and not F[2].any() and rc_ab(3.4)[0, 2] == 0
    assert np.array_equal(pair_table.knots(R_MIN, R_MAX, NK)[[0, -1]], [R_MIN, R_MAX])


def test_sample_and_interpolate_converge():
    """An LJ table against Lennard-Jones itself: per pair within D^2 max |F_xx| / 8 of the segment, falling 4 x per doubling of
    nknots; summed per particle within the sum of those bounds of lj_reference."""
    box6, mask = LJ_BOXES["xyz"]
    q, pairs = _input("xyz", False), _pairs("xyz", False)
    want, _ = lj_reference(q, box6, mask, 1.0, 1.0, R_MAX, pairs=pairs)
    worst = []
    for nk in (256, 512, 1024, 2048):
        F, U = pair_table.sample(*lj(), R_MIN, R_MAX, nk)
        D = pair_table.spacing(R_MIN, R_MAX, nk)
        I, J, d, fr, pe, _, _ = table_pairs(q, F, U, R_MIN, R_MAX, pairs)
        r2 = (d * d).sum(axis=1)
        exact = 24.0 * (2.0 * r2 ** -7.0 - r2 ** -4.0)
        bound = _lj_interp_bound(r2, D, lj_f_xx)
        assert np.all(np.abs(fr - exact) <= bound)
        x = np.linspace(0.92 ** 2, R_MAX ** 2, 200001)[:-1]  # (a dense grid: the largest error does not hang on where pairs fall)
        worst.append(np.abs(pair_table.interpolate(F, U, R_MIN, R_MAX, x)[0] - 24.0 * (2.0 * x ** -7.0 - x ** -4.0)).max())
        got, _ = table_reference(q, box6, mask, F, U, R_MIN, R_MAX, pairs=pairs)
        for c in range(3):
            assert np.all(np.abs(got[:, c] - want[:, c]) <= np.bincount(I, weights=bound * np.abs(d[:, c]), minlength=N))
        assert np.all(np.abs(got[:, 3] - want[:, 3]) <= np.bincount(I, weights=0.5 * _lj_interp_bound(r2, D, lj_u_xx), minlength=N))
    ratios = np.array(worst[:-1]) / np.array(worst[1:])
    print("largest pair error per nknots", worst, "ratios", ratios)
    assert np.all((ratios > 3.0) & (ratios < 5.0))


def _lj_interp_bound(r2, D, f_xx):
    """D^2 max |f_xx| / 8 over the segment of each r2 (|f_xx| is monotone on a segment but for one extremum, which the factor
    1.02 covers at these spacings), plus a few float64 roundings."""
    k = np.floor((r2 - R_MIN ** 2) / D)
    lo, hi = R_MIN ** 2 + k * D, R_MIN ** 2 + (k + 1) * D
    return 1.02 * D * D / 8.0 * np.maximum(np.abs(f_xx(lo)), np.abs(f_xx(hi))) + 1e-13


def test_reference_is_the_gradient_of_its_energy():
    """table_reference's forces against the central difference of its own total energy, tilted and periodic, two types.  The
    potentials are U = b (r_max^2 - r^2), linear in r^2: both tables interpolate them exactly, and they vanish at r_max, so the
    energy has no jump there and the forces are its gradient to rounding."""
    rng = np.random.default_rng(3)
    m, a = 5, 1.125
    box6, mask = (m * a, m * a, m * a, a, -a, 2 * a), 7
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (g + 0.5) * a + rng.uniform(-0.1, 0.1, size=g.shape)
    r_max, h = 1.8, 1e-5
    types = rng.integers(0, 2, size=len(q))
    b = (1.0, 1.7, 0.6)  # slots (0, 0), (0, 1), (1, 1)
    rows = [pair_table.sample(lambda r, v=v: v * (r_max ** 2 - r * r), lambda r, v=v: -2.0 * v * r, 0.5, r_max, 64) for v in b]
    F, U = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert np.allclose(F, 2.0 * np.array(b)[:, None])
    want, S = table_reference(q, box6, mask, F, U, 0.5, r_max, types=types)
    for i in range(4):
        for c in range(3):
            e = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                e.append(table_reference(p, box6, mask, F, U, 0.5, r_max, types=types)[0][:, 3].sum())
            fd = -(e[0] - e[1]) / (2 * h)
            assert abs(fd - want[i, c]) <= 1e-6 * S[i, c], (i, c, fd, want[i, c])
    assert np.abs(want[:, :3].sum(axis=0)).max() <= 1e-12 * S[:, :3].sum()  # Newton's third law in the reference
    w, SW = table_virial_reference(q, box6, mask, F, U, 0.5, r_max, types=types)
    assert abs(w[6] - want[:, 3].sum()) <= 1e-12 * SW[6] and w[7] > len(q)


def test_emulation_gives_c():
    """TABLE_C and TABLE_CW = 4 x the largest |emulated - want| / (u S) of a numpy emulation of the kernel's arithmetic
    (never the kernel) against the float64 reference: 2.67 per particle and component (fy; energies 2.42), 0.487 for the totals (W_yy in fp64, one ulp of the sum; 0.197 in fp32)."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    for box, drift, tab in EMULATED:
        box6, mask = LJ_BOXES[box]
        F, U, types, _ = _tab(tab)
        (want, S), (ww, SW) = _ref(box, drift, tab)
        I, J = _pairs(box, drift)[:2]
        if types is not None:  # (the pairs the type table leaves out of the list)
            keep = ~(((types[I] == 0) & (types[J] == 2)) | ((types[I] == 2) & (types[J] == 0)))
            I, J = I[keep], J[keep]
        q = _input(box, drift)
        vals = {T: table_emulate_pairs(q, box6, mask, F, U, R_MIN, R_MAX, T, (I, J), types=types) for T in DTYPES}
        for order in range(3):
            rng = np.random.default_rng(100 + order)
            f = table_emulate(q, box6, mask, F, U, R_MIN, R_MAX, np.float32, rng, (I, J), types=types)
            r = lj_ratio(f, want, S, np.float32).max(axis=0)
            rw = []
            for T in DTYPES:  # (the totals are summed in double whatever T is: in fp64 that sum is the error)
                w = table_virial_emulate(N, I, vals[T], rng)
                assert w[7] == ww[7]
                rw.append(virial_ratio(w, ww, SW, T))
            print(box, drift, tab, order, r.round(2), rw[0].round(2), rw[1].round(2))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, np.maximum(*rw))
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX <= TABLE_C / 4
    assert worst_w.max() <= EMULATED_MAX_W <= TABLE_CW / 4


def test_bound_is_sharp():
    """On every input TABLE_C u S stays below a quarter of what the weakest single pair at r_max gives a component."""
    seen = 0
    for box, drift in CASES:
        for tab in TABS:
            _assert_sharp(_ref(box, drift, tab), tab)
            seen += 1
    for box in ("xyz", "tilt"):
        for tab in ("morse", "typed3"):
            _assert_sharp(_moved_ref(box, tab), tab)
    assert seen == 27


def test_wrong_results_are_rejected():
    """check_lj under the fp32 bound refuses: one pair dropped, a neighbouring knot, t ignored, the reaction missing."""
    box6, mask = LJ_BOXES["xyz"]
    q, pairs = _input("xyz", False), _pairs("xyz", False)
    for tab in ("morse", "lj"):
        F, U, _, _ = _tab(tab)
        (want, S), (ww, SW) = _ref("xyz", False, tab)
        check_lj(want, want, S, np.float32, c=TABLE_C)
        I, J, d, fr, pe, _, _ = table_pairs(q, F, U, R_MIN, R_MAX, pairs)
        r2 = (d * d).sum(axis=1)
        wrong = {}
        k = int(np.argmax(r2))  # the weakest pair: the one closest to r_max, dropped from both its particles
        w = want.copy()
        for i, sgn in ((I[k], 1.0), (J[k], -1.0)):
            w[i, :3] -= sgn * fr[k] * d[k]
            w[i, 3] -= 0.5 * pe[k]
        wrong["one pair dropped"] = w
        rng = np.random.default_rng(5)
        for name, defect in (("the knot below", dict(knot_shift=-1)), ("the knot above", dict(knot_shift=1)), ("t ignored", dict(use_t=False))):
            wrong[name] = table_emulate(q, box6, mask, F, U, R_MIN, R_MAX, np.float64, rng, pairs[:2], **defect)
        half = I < J  # a half list without the reaction: every pair reaches the particle of the smaller id only
        w = np.zeros((N, 4))
        for c in range(3):
            w[:, c] = np.bincount(I[half], weights=fr[half] * d[half, c], minlength=N)
        w[:, 3] = np.bincount(I[half], weights=0.5 * pe[half], minlength=N)
        wrong["the reaction missing"] = w
        good = table_emulate(q, box6, mask, F, U, R_MIN, R_MAX, np.float64, rng, pairs[:2])
        check_lj(good, want, S, np.float32, c=TABLE_C)
        for name, w in wrong.items():
            with pytest.raises(AssertionError):
                check_lj(w, want, S, np.float32, c=TABLE_C)
            assert name
        wv = ww.copy()  # the totals, whose S sums over every pair of the box: the weakest pair dropped, under the fp64 bound
        wv[:3] -= fr[k] * d[k] * d[k]
        wv[6] -= pe[k]
        with pytest.raises(AssertionError):
            check_virial(wv, ww, SW, np.float64, c=TABLE_CW, count=False)


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _set(nl, tab, rc, nk=NK):
    """The table (and, for a typed one, the type table at the list's cut-off) onto a handle that has been initialised."""
    F, U, types, rc_ab = _tab(tab, nk)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab(rc))
    nl.set_pair_table(F, U, R_MIN, R_MAX)


def _check(f, w, refs, dtype, rows=None):
    (want, S), (ww, SW) = refs
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, want, S, dtype).max(axis=0).round(2), virial_ratio(w, ww, SW, dtype).round(2))
    check_lj(f, want, S, dtype, c=TABLE_C, rows=rows)
    if rows is None:
        check_virial(w, ww, SW, dtype, c=TABLE_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (TABLE_C + TABLE_CW) * lj_unit(dtype) * SW[6]
    return f, w


TABLE = contract.Consumer(
    forces="table_forces", virial="table_virial", scratch="table_virial", clear="clear_pair_table", info="pair_table",
    entry=("nl_table_forces", "nl_table_forces_enqueue", "nl_table_virial", "nl_table_virial_enqueue"), set=_set, kinds=TABS, ref=_ref,
    moved_ref=_moved_ref, extra=lambda nl: (), check=lambda f, w, x, refs, dtype, rows=None: _check(f, w, refs, dtype, rows),
    half_lists=True, local_slabs=True)
_built = functools.partial(contract.built, TABLE)
gpu = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x Morse, LJ and the 3-type table x list kind x dtype; the list cut-off, the offset
    width and q_stride rotate through the cases.  Two calls of the totals are bit-identical."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, tab in enumerate(TABS):
        k = case + p + (1 if full else 0)
        rc, off, stride = RC_LISTS[k % 2], (32, 64)[(k // 2 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        nl, qd = _built(q, box, dtype, full, rc, tab, off, stride)
        assert nl.pair_table() == dict(ntypes=1 if tab != "typed3" else 3, nknots=NK, r_min=R_MIN, r_max=R_MAX)
        f, w = nl.table_forces(qd), nl.table_virial(qd)
        assert f.shape == (N, 4) and f.dtype == _tdt(dtype) and w.shape == (8,) and w.dtype == _torch().float64
        _, w = _check(f, w, _ref(box, drift, tab), dtype)
        assert w.tobytes() == nl.table_virial(qd).cpu().numpy().tobytes() and len(w.tobytes()) == 64


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,tab", [("tilt", True, "typed3"), ("xyz", False, "morse")])
def test_half_and_full_agree(box, drift, tab, dtype):
    refs = _ref(box, drift, tab)
    got = {}
    for full in (False, True):
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, tab)
        got[full] = _check(nl.table_forces(qd), nl.table_virial(qd), refs, dtype)
    u = lj_unit(dtype)
    assert np.all(np.abs(got[False][0].astype(np.float64) - got[True][0]) <= 2 * TABLE_C * u * refs[0][1])
    assert np.all(np.abs(got[False][1][:7] - got[True][1][:7]) <= 2 * TABLE_CW * u * refs[1][1])
    assert got[False][1][7] == got[True][1][7] == refs[1][0][7]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tab,nk", [("morse", NK), ("typed3", 256)])
def test_lds_and_global_paths(tab, nk, dtype, monkeypatch):
    """A table set under NL_TABLE_LDS=0 is read from global memory.  On one list -- the order of the partners in a row varies
    from build to build, and with it the last bits of any sum over them -- the two paths give the same bits: full-list
    forces and the totals of both list kinds; half-list forces within the bound (their atomics fix no order).  A fresh handle
    created, built and set under the switch stays within the bound as well."""
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    lds_bytes = int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1))
    assert np.atleast_2d(_tab(tab, nk)[0]).size * 4 * np.dtype(dtype).itemsize <= lds_bytes  # staged unless switched off
    box, drift = "tilt", True
    refs = _refs(_input(box, drift), box, tab, _pairs(box, drift), nk)
    for full in (False, True):
        monkeypatch.delenv("NL_TABLE_LDS", raising=False)
        nl, qd = _built(_input(box, drift), box, dtype, full, 3.4, tab, nk=nk)
        lds = _check(nl.table_forces(qd), nl.table_virial(qd), refs, dtype)
        monkeypatch.setenv("NL_TABLE_LDS", "0")
        nl.set_pair_table(*_tab(tab, nk)[:2], R_MIN, R_MAX)  # (the same table, the same list: the other path)
        glo = _check(nl.table_forces(qd), nl.table_virial(qd), refs, dtype)
        assert lds[1].tobytes() == glo[1].tobytes() and len(glo[1].tobytes()) == 64
        if full:
            assert lds[0].tobytes() == glo[0].tobytes()
        fresh, qf = _built(_input(box, drift), box, dtype, full, 3.4, tab, nk=nk)
        _check(fresh.table_forces(qf), fresh.table_virial(qf), refs, dtype)


@gpu
def test_a_large_table_takes_the_global_path():
    """32 types x 4096 knots: 528 slots, 34.6 MB in fp32 -- far beyond NL_TABLE_LDS_BYTES."""
    nt, nk = 32, 4096
    types = lj_type_params(nt, 3.4)[0]
    rows = [pair_table.sample(*morse(De=1.0 + 0.2 * (s % 5), a=1.5, r0=1.05 + 0.03 * (s % 6)), R_MIN, R_MAX, nk) for s in range(30)]
    F = np.stack([rows[s % 30][0] for s in range(rdf.nslots(nt))])
    U = np.stack([rows[s % 30][1] for s in range(rdf.nslots(nt))])
    box, dtype = "xyz", np.float32
    box6, mask = LJ_BOXES[box]
    q = _input(box, True)
    kw = dict(pairs=_pairs(box, True), types=types)
    refs = (table_reference(q, box6, mask, F, U, R_MIN, R_MAX, **kw), table_virial_reference(q, box6, mask, F, U, R_MIN, R_MAX, **kw))
    for full in (False, True):
        nl = _handle(box, dtype, full, 2.5)
        nl.Initialize(N)
        nl.set_type_cutoffs(types, np.full((nt, nt), 2.5))
        nl.set_pair_table(F, U, R_MIN, R_MAX)
        assert nl.pair_table()["ntypes"] == nt
        qd = _torch().from_numpy(q.astype(dtype)).cuda()
        nl.MakeNeighList(qd, N)
        _check(nl.table_forces(qd), nl.table_virial(qd), refs, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_an_lj_table_is_nl_lj_forces(full, dtype):
    """A 4096-knot LJ table against nl_lj_forces on the same list: within the interpolation bound of the table (from F_xx and
    U_xx, test_sample_and_interpolate_converge) plus both rounding bounds."""
    nk, box, drift = 4096, "xyz", True
    box6, mask = LJ_BOXES[box]
    q, pairs = _input(box, drift), _pairs(box, drift)
    nl, qd = _built(q, box, dtype, full, 3.4, "lj", nk=nk)
    ft = nl.table_forces(qd).cpu().numpy().astype(np.float64)
    fl = nl.lj_forces(qd, 1.0, 1.0, rc_force=R_MAX).cpu().numpy().astype(np.float64)
    F, U, _, _ = _tab("lj", nk)
    D = pair_table.spacing(R_MIN, R_MAX, nk)
    I, J, d, _, _, _, _ = table_pairs(q, F, U, R_MIN, R_MAX, pairs)
    r2 = (d * d).sum(axis=1)
    St = table_reference(q, box6, mask, F, U, R_MIN, R_MAX, pairs=pairs)[1]
    Sl = lj_reference(q, box6, mask, 1.0, 1.0, R_MAX, pairs=pairs)[1]
    u = lj_unit(dtype)
    bound = TABLE_C * u * St + LJ_C * u * Sl
    for c in range(3):
        bound[:, c] += np.bincount(I, weights=_lj_interp_bound(r2, D, lj_f_xx) * np.abs(d[:, c]), minlength=N)
    bound[:, 3] += np.bincount(I, weights=0.5 * _lj_interp_bound(r2, D, lj_u_xx), minlength=N)
    print((np.abs(ft - fl) / bound).max(axis=0))
    assert np.all(np.abs(ft - fl) <= bound)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_a_pair_below_the_table(full, dtype):
    """One particle moved to 0.5 from its neighbour, below r_min: NaN in exactly those two particles' forces and energies (half
    list: the row and the reaction; full list: each one's own row), 8 NaN totals, everybody else within the bound."""
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
    refs = _refs(q, box, "morse", pairs)
    nans = np.isnan(refs[0][0]).all(axis=1)
    assert np.array_equal(np.flatnonzero(nans), sorted((a, b))) and np.isnan(refs[1][0]).all()
    nl, qd = _built(q, box, dtype, full, 2.5, "morse")
    f, w = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,)
    assert np.array_equal(np.isnan(f), np.repeat(nans[:, None], 4, axis=1))
    check_lj(f, *refs[0], dtype, c=TABLE_C, rows=~nans)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,tab", [("xyz", "morse"), ("tilt", "typed3")])
def test_reuse_within_the_skin(box, tab, full, dtype):
    contract.reuse_within_the_skin(TABLE, box, tab, full, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """One graph holds the copy of the positions, the update, the forces and the totals; replayed at two position sets.  A
    table of the same size set afterwards keeps the device buffer: the next replay computes with the new table."""
    def before(nl, qd, fd, wd):
        nl.table_virial(qd, wait=False, out=wd)  # once before the capture: the scratch exists
        nl.synchronize()

    def after(nl, replay):
        nl.set_pair_table(*_tab("lj")[:2], R_MIN, R_MAX)
        _check(*replay(), _moved_ref("xyz", "lj"), np.float32)

    contract.captured(TABLE, full, before, after)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN forces and 8 NaN totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat both are finite."""
    def set_tables(nl):
        F, U = pair_table.sample(*morse(), 1e-3, R_MAX, NK)  # (a uniform random box has close pairs: the table starts near 0)
        nl.set_pair_table(F, U, 1e-3, R_MAX)

    contract.failed_list(TABLE, set_tables, lambda nl, qd: None)  # (no scratch before the capacity shrinks)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("layers", [((0, 2), (2, 4)), ((0, 1), (1, 3), (3, 4))])
@pytest.mark.parametrize("box,drift", [("xyz", True), ("open", False)])
def test_local_index_slabs(box, drift, layers, full, dtype):
    """2 and 3 slabs, one after the other on the one device: every owned particle's force within the bound of the whole-box
    reference, the ranks' 8 doubles add up to the whole-box totals within the bound, n_in exactly."""
    from tests.test_slab_paths import slab_parts

    torch = _torch()
    rc = 3.4
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    (want, S), (ww, SW) = _ref(box, drift, "morse")
    parts = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, layers, mask)
    assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(N))
    nl = _handle(box, dtype, full, rc)
    nl.set_local_ids(True)
    nl.Initialize(N)
    _set(nl, "morse", rc)
    tot = np.zeros(8)
    for part in parts:
        qd = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
        nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"])
        f, w = nl.table_forces(qd).cpu().numpy(), nl.table_virial(qd).cpu().numpy()
        assert f.shape == (len(part["own"]), 4)
        check_lj(f, want[part["own"]], S[part["own"]], dtype, c=TABLE_C)
        tot += w
    check_virial(tot, ww, SW, dtype, c=TABLE_CW)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    F, U, _, _ = _tab("morse")
    F3, U3, types, _ = _tab("typed3")
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    calls = contract.entry_calls(TABLE, lib, fd, out)
    set_one = lambda: nl.set_pair_table(F, U, R_MIN, R_MAX)  # noqa: E731
    # no table: the getter, the wrapper, and the calls after a build
    assert nl.pair_table() is None
    assert lib.nl_get_pair_table(nl._h, None, None, None, None) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for fn, o in calls:
        assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    # the setter's arguments: each refused, and the table that was set is kept
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    want = nl.table_virial(qd).cpu().numpy()  # (reproducible bit for bit; a half list's forces are not)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    bad_f = F.copy()
    bad_f[7] = np.inf
    bad_u = U.copy()
    bad_u[-1] = np.nan
    big = np.zeros(4097)
    for args in ((1, NK, R_MIN, R_MAX, dp(F), None), (1, NK, R_MIN, R_MAX, None, dp(U)), (1, 1, R_MIN, R_MAX, dp(F), dp(U)),
                 (1, -3, R_MIN, R_MAX, dp(F), dp(U)), (1, 4097, R_MIN, R_MAX, dp(big), dp(big)), (1, NK, 0.0, R_MAX, dp(F), dp(U)),
                 (1, NK, -1.0, R_MAX, dp(F), dp(U)), (1, NK, R_MAX, R_MAX, dp(F), dp(U)), (1, NK, R_MIN, np.inf, dp(F), dp(U)),
                 (1, NK, np.nan, R_MAX, dp(F), dp(U)), (0, NK, R_MIN, R_MAX, dp(F), dp(U)), (33, NK, R_MIN, R_MAX, dp(F), dp(U)),
                 (1, NK, R_MIN, R_MAX, dp(bad_f), dp(U)), (1, NK, R_MIN, R_MAX, dp(F), dp(bad_u))):
        assert lib.nl_set_pair_table(nl._h, *args) == NL_ERR_ARG, args[:4]
        assert nl.pair_table() == dict(ntypes=1, nknots=NK, r_min=R_MIN, r_max=R_MAX)
    assert lib.nl_set_pair_table(None, 1, NK, R_MIN, R_MAX, dp(F), dp(U)) == NL_ERR_ARG
    assert nl.table_virial(qd).cpu().numpy().tobytes() == want.tobytes() and np.isfinite(want).all()
    with pytest.raises(TypeError):
        nl.set_pair_table(F, U[:-1], R_MIN, R_MAX)
    with pytest.raises(TypeError):
        nl.set_pair_table(np.zeros((4, 8)), np.zeros((4, 8)), R_MIN, R_MAX)  # 4 rows are no ntypes (ntypes + 1) / 2
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_one)
    contract.reach(TABLE, nl, qd, lambda r_max: nl.set_pair_table(*pair_table.sample(*morse(), R_MIN, r_max, NK), R_MIN, r_max))
    set_one()
    contract.clearing(TABLE, nl, qd, set_one, lambda: lib.nl_set_pair_table(nl._h, 1, 0, R_MIN, R_MAX, dp(F), dp(U)))
    contract.several_types(TABLE, nl, qd, types, set_one, lambda: nl.set_pair_table(F3, U3, R_MIN, R_MAX))
    # a first call of the totals inside a capture, on a handle whose scratch does not exist yet
    fresh = _handle("open", np.float32, False, 2.9)
    fresh.Initialize(N)
    fresh.set_pair_table(F, U, R_MIN, R_MAX)
    fresh.MakeNeighList(qd, N)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(NLError) as e:
            fresh.table_virial(qd, wait=False)
        fresh.table_forces(qd, wait=False, out=fd)
    assert e.value.code == NL_ERR_STATE
    contract.no_particles(TABLE, lib, False, lambda empty: empty.set_pair_table(F, U, R_MIN, R_MAX), qd, fd, out)

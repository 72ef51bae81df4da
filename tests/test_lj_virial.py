"""nl_lj_virial, nl_lj_virial_typed and their enqueue variants: the virial tensor, the potential energy and the number of
interacting pairs from the list, against an O(N^2) float64 sum that uses no list (tests.virial_util virial_reference).

Contract tested (include/nl_hip.h, nl_lj_virial):
  * |got - want| <= c_W u S for each of W_xx, W_yy, W_zz, W_xy, W_xz, W_yz and U on its own: S the uncancelled sum of that
    component's pair terms, u = 2^-24 (fp32) or 2^-53 (fp64);
  * n_in exactly, for both dtypes: every input keeps its pairs 2^-17 (relative, r^2) away from every cut-off;
  * half and full lists report the same totals; two calls return the same 64 bytes.

c_W = VIR_C = 4 x the largest per-row ratio |emulated row sum - float64 row sum| / (u S_row) that a float32 numpy
emulation of the kernel's arithmetic reaches (emulate_pairs, which lj_emulate sums too; virial_emulate: the six products
and the energy in float32, one rounding each, converted and added in double as the kernel adds them) over the nine
inputs of EMULATED, both list kinds, three summation orders; test_emulation_gives_c recomputes the maximum.  The totals
are double sums of such row values, so the per-row bound carries over by the triangle inequality; the factor 4 is section
8j's (another summation tree, the host's rounding of the parameters and the box).  The kernel adds in double, so the
rows' error is that of the terms alone and c_W comes out below LJ_C.

What the bound catches.  A single pair has no least contribution to one component (d_x can vanish), but it has to the
trace, r F, and to U.  fp64: c_W u S is about 1e-9 while one pair at rc_force gives |r F| = 0.0975 (eps = sigma = 1,
rc_force = 2.5): test_bound_is_sharp asserts c_W u (S_xx + S_yy + S_zz) <= 1/4 |r F(rc_force)| and c_W u S_U <= 1/4
|U(rc_force)| of the weakest type pair on every input, so no pair can go missing under the fp64 bound.  fp32: on the
lattice c_W u S is wider than one weak pair; there n_in, compared exactly, carries the structural check.  On the dimer
input the 1/4 condition holds for fp32 too and is asserted.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests.consumer_util import BIG_BOX, CASES, DTYPES, EMULATED, N, PARS, RC_LISTS, RCF, _big, _bonds, _dimers, _handle, _tdt, _torch
from tests.consumer_util import NBLK_VIRIAL as NBLK
from tests.consumer_util import _lj_forces as _forces
from tests.consumer_util import _lj_input as _input
from tests.consumer_util import _lj_moved as _moved
from tests.consumer_util import _lj_moved_pairs as _moved_pairs
from tests.consumer_util import _lj_pairs as _pairs
from tests.consumer_util import _lj_par as _par
from tests.util import LJ_BOXES, LJ_C, LJ_L, ROOT, lj_band_particles, lj_drift, lj_emulate, lj_pairs, lj_unit
from tests.virial_util import VIR_C, check_virial, emulate_pairs, virial_emulate, virial_ratio, virial_reference

EMULATED_MAX = 11.9  # the largest per-row ratio of test_emulation_gives_c


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _vref(box, drift, par, shift=False):
    box6, mask = LJ_BOXES[box]
    types, _, eps, sig, rcf = _par(par)
    return virial_reference(_input(box, drift, shift), box6, mask, eps, sig, rcf, types=types, pairs=_pairs(box, drift, shift))


@functools.lru_cache(maxsize=None)
def _excluded_vref():
    box6, mask = LJ_BOXES["xyz"]
    return virial_reference(_input("xyz", False), box6, mask, 1.0, 1.0, RCF, exclusions=_bonds(), pairs=_pairs("xyz", False))


@functools.lru_cache(maxsize=None)
def _moved_vref(box, par, seed=21):
    box6, mask = LJ_BOXES[box]
    types, _, eps, sig, rcf = _par(par)
    pairs = _moved_pairs(box) if seed == 21 else lj_pairs(_moved(box, 0.03, seed), box6, mask, RCF)
    return virial_reference(_moved(box, 0.03, seed), box6, mask, eps, sig, rcf, types=types, pairs=pairs)


def _weakest(par):
    """(|r F(rc_force_ab)|, |U(rc_force_ab)|) of the weakest pair of types: the least a single pair adds to the trace and
    to the energy."""
    _, _, eps, sig, rcf = _par(par)
    eps, sig, rcf = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (eps, sig, rcf))
    live = rcf > 0
    s6 = (sig / np.where(live, rcf, 1.0)) ** 6
    rF = np.where(live, np.abs(24.0 * eps * (2.0 * s6 * s6 - s6)), np.inf).min()
    U = np.where(live, np.abs(4.0 * eps * (s6 * s6 - s6)), np.inf).min()
    return rF, U


def _assert_sharp(S, par, dtype):
    rF, U = _weakest(par)
    u = lj_unit(dtype)
    assert VIR_C * u * S[:3].sum() <= 0.25 * rF, (VIR_C * u * S[:3].sum(), rF)
    assert VIR_C * u * S[6] <= 0.25 * U, (VIR_C * u * S[6], U)


DIMER_BOXES = {"open": ((63.0, 63.0, 63.0, 0.0, 0.0, 0.0), 0), "xyz": ((63.0, 63.0, 63.0, 0.0, 0.0, 0.0), 7),
               "tilt": ((63.0, 63.0, 63.0, 10.5, -10.5, 21.0), 7)}


def _dimer_inputs(box, dtype):
    """[(q, group)]: the dimers in the box and, in a periodic box, moved apart by whole lattice vectors."""
    box6, mask = DIMER_BOXES[box]
    base, group, inner = _dimers(dtype, box6, mask)
    if not mask:
        return [(base, group)]
    shifts = np.random.default_rng(9).integers(-1, 2, size=(len(base), 3))
    shifts[2 * inner[:20]], shifts[2 * inner[:20] + 1] = (-1, 0, 1), (1, 0, -1)
    return [(base, group), (lj_drift(base, 0, (box6, mask), k=shifts), group)]


# ------------------------------------------------------------------------------------------------- CPU: the checker
def test_header_states_the_block_cap():
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    assert int(re.search(r"#define NL_VIRIAL_BLOCKS (\d+)", text).group(1)) == NBLK <= 2048
    assert len(_input("xyz", False)) * 4 > 4 * NBLK


def _strained(q, box6, M):
    """Positions and box under the homogeneous deformation r -> M r, M upper triangular (the box keeps its form)."""
    Lx, Ly, Lz, xy, xz, yz = box6
    H = M @ np.array([[Lx, xy, xz], [0.0, Ly, yz], [0.0, 0.0, Lz]])
    p = q.copy()
    p[:, :3] = q[:, :3] @ M.T
    return p, (H[0, 0], H[1, 1], H[2, 2], H[0, 1], H[0, 2], H[1, 2])


def test_reference_is_the_strain_derivative_of_its_energy():
    """W_ab = -dU/d(eps_ab) of virial_reference's own energy, by central differences with h = 1e-5, on a 5^3 tilted,
    periodic, two-type lattice; and tr W = -3 V dU/dV.  The deformation applied is r -> (I + h e_a e_b^T) r with a <= b:
    the symmetrised strain differs from it by a rotation to first order, which U does not see, and this one keeps
    the box in the form (Lx, Ly, Lz, xy, xz, yz) that the reference takes."""
    rng = np.random.default_rng(3)
    m, a = 5, 1.125
    box6, mask = (m * a, m * a, m * a, a, -a, 2 * a), 7
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    site = (g + 0.5) * a
    q = np.zeros((len(g), 4))
    q[:, :3] = site + rng.uniform(-0.1, 0.1, size=site.shape)
    rcf, h = 2.2, 1e-5
    for _ in range(20):  # no pair within 1e-3 (relative, r^2) of the cut-off: a pair crossing it is a jump in U
        bad = lj_band_particles(q, box6, mask, (rcf,), 1e-3)
        if not len(bad):
            break
        q[bad, :3] = site[bad] + rng.uniform(-0.1, 0.1, size=(len(bad), 3))
    assert not len(lj_band_particles(q, box6, mask, (rcf,), 1e-3))
    types = rng.integers(0, 2, size=len(q))
    eps, sig = np.array([[1.0, 1.7], [1.7, 0.6]]), np.array([[1.0, 0.95], [0.95, 1.05]])

    def energy(M):
        p, b6 = _strained(q, box6, M)
        return virial_reference(p, b6, mask, eps, sig, rcf, types=types)[0][6]

    def derivative(E):
        return (energy(np.eye(3) + h * E) - energy(np.eye(3) - h * E)) / (2 * h)

    want, S, _ = virial_reference(q, box6, mask, eps, sig, rcf, types=types)
    assert want[7] > 1000 and np.all(S > 0)
    for k, (ia, ib) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        E = np.zeros((3, 3))
        E[ia, ib] = 1.0
        fd = -derivative(E)
        assert abs(fd - want[k]) <= 1e-6 * S[k], (k, fd, want[k])
    # isotropic: V = (1 + h)^3 V0, so dU/dh = 3 V dU/dV
    assert abs(-derivative(np.eye(3)) - want[:3].sum()) <= 1e-6 * S[:3].sum()


def test_emulation_is_lj_emulate():
    """tests.util lj_emulate is emulate_pairs and a row sum: with one entry per row, where nothing is summed, it returns
    f = {fx, fy, fz, pe / 2} of the pair's values, bit for bit, on every box form."""
    for box, drift, par in (("tilt", True, "typed32"), ("xyz", True, "scalar"), ("open", False, "scalar")):
        box6, mask = LJ_BOXES[box]
        types, _, eps, sig, rcf = _par(par)
        I, J = _vref(box, drift, par)[2]["full"][:2]
        first = np.unique(I, return_index=True)[1]
        I, J = I[first], J[first]
        vals = emulate_pairs(_input(box, drift), box6, mask, eps, sig, rcf, np.float32, (I, J), types=types)
        f = lj_emulate(_input(box, drift), box6, mask, eps, sig, rcf, np.float32, np.random.default_rng(0), (I, J), types=types)
        assert vals[7].all() and len(I) == N
        assert np.array_equal(f[I], np.stack([vals[3], vals[4], vals[5], np.float32(0.5) * vals[6]], axis=1))


def test_emulation_gives_c():
    """c_W = 4 x the largest per-row |emulated - want| / (u S_row) of a float32 emulation of the kernel's arithmetic (never
    the kernel); the emulated totals themselves stay within 1 u S, and their n_in is the reference's."""
    worst, worst_total = np.zeros(7), 0.0
    for box, drift, par in EMULATED:
        box6, mask = LJ_BOXES[box]
        types, _, eps, sig, rcf = _par(par)
        want, S, rows = _vref(box, drift, par)
        for kind, scale in (("half", 1.0), ("full", 0.5)):
            I, J, row, S_row = rows[kind]
            vals = emulate_pairs(_input(box, drift), box6, mask, eps, sig, rcf, np.float32, (I, J), types=types)
            for order in range(3):
                got, n_in = virial_emulate(N, I, vals, np.random.default_rng(100 + order))
                r = virial_ratio(got, row, S_row, np.float32).max(axis=0)
                total = virial_ratio(scale * got.sum(axis=0), want, S, np.float32).max()
                print(box, drift, par, kind, order, r.round(2), round(float(total), 3))
                worst, worst_total = np.maximum(worst, r), max(worst_total, total)
                assert scale * n_in == want[7]
    print("largest per-row ratio per column", worst, "largest ratio of the totals", worst_total)
    assert worst.max() <= EMULATED_MAX and 4 * EMULATED_MAX <= VIR_C
    assert worst_total <= 1.0


def test_bound_is_sharp():
    """fp64: c_W u S is below a quarter of the weakest single pair's r F and U on every input; fp32: on the dimers."""
    seen = 0
    for box, drift in CASES:
        for par in PARS:
            _assert_sharp(_vref(box, drift, par)[1], par, np.float64)
            seen += 1
    assert seen == 27
    for box in ("xyz", "tilt"):
        for par in ("scalar", "typed3"):
            _assert_sharp(_moved_vref(box, par)[1], par, np.float64)
    _assert_sharp(_excluded_vref()[1], "scalar", np.float64)
    rF, U = _weakest("scalar")
    assert abs(rF - 0.0975) < 5e-4 and abs(U - 0.01632) < 1e-5
    S = _vref("xyz", False, "scalar")[1]
    assert VIR_C * lj_unit(np.float64) * S.max() < 1e-8
    assert VIR_C * lj_unit(np.float32) * S[:3].sum() > rF  # (fp32 on the lattice: wider than one weak pair; n_in decides)
    for box, (box6, mask) in DIMER_BOXES.items():
        for dtype in DTYPES:
            for q, _ in _dimer_inputs(box, dtype):
                _assert_sharp(virial_reference(q, box6, mask, 1.0, 1.0, RCF)[1], "scalar", dtype)


def test_wrong_results_are_rejected():
    """check_virial on float64 results with one deliberate defect each, under the fp64 bound and without the help of
    n_in: every one is refused.  And n_in off by one is refused for fp32."""
    box6, mask = LJ_BOXES["xyz"]
    q, (I, J, d, raw) = _input("xyz", False), _pairs("xyz", False)
    want, S, _ = _vref("xyz", False, "scalar")
    check_virial(want, want, S, np.float64)

    def term(dk):  # one pair's contribution to the 7 sums
        r2 = (dk * dk).sum()
        s6 = 1.0 / r2 ** 3
        fr = 24.0 * (2.0 * s6 * s6 - s6) / r2
        return np.array([fr * dk[0] * dk[0], fr * dk[1] * dk[1], fr * dk[2] * dk[2], fr * dk[0] * dk[1], fr * dk[0] * dk[2],
                         fr * dk[1] * dk[2], 4.0 * (s6 * s6 - s6), 1.0])

    wrong = {}
    r2 = (d * d).sum(axis=1)
    inn = r2 < RCF * RCF
    k = int(np.flatnonzero(inn)[np.argmax(r2[inn])])
    wrong["the weakest pair dropped"] = want - term(d[k])
    wrong["a full list without the 1/2"] = 2.0 * want
    wrong["W_xy and W_xz swapped"] = want[[0, 1, 2, 4, 3, 5, 6, 7]]
    wrong["cut at the list's rc"] = virial_reference(q, box6, mask, 1.0, 1.0, 3.4, pairs=(I, J, d, raw))[0]
    k = int(np.flatnonzero(inn & (np.abs(raw).max(axis=1) > 0.5 * LJ_L))[0])  # beyond rc_force at its raw coordinates
    wrong["a face-crossing pair at raw coordinates"] = want - term(d[k])
    for name, w in wrong.items():
        with pytest.raises(AssertionError):
            check_virial(w, want, S, np.float64, count=False)
        assert name
    w = want.copy()
    w[7] += 1.0
    check_virial(w, want, S, np.float32, count=False)
    with pytest.raises(AssertionError, match="n_in"):
        check_virial(w, want, S, np.float32)
    w = want.copy()
    w[2] = np.nan
    with pytest.raises(AssertionError, match="zz"):
        check_virial(w, want, S, np.float32)


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _virial(nl, qd, par, **kw):
    """The wrapper call of a parameter set (after _forces, which sets the tables), as a device tensor."""
    return nl.lj_virial_typed(qd, **kw) if par != "scalar" else nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF, **kw)


def _check_energy(w, f, S, dtype):
    """U against the sum of nl_lj_forces' pe_i: each within its own bound of the same float64 value."""
    pe = f[:, 3].astype(np.float64).sum()
    assert abs(w[6] - pe) <= (VIR_C + LJ_C) * lj_unit(dtype) * S[6], (w[6], pe)


# -------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x scalar and typed parameters x list kind x dtype; list cut-off, offset width
    and q_stride rotate as in test_lj_consumer's test_matrix."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, par in enumerate(PARS):
        k = case + p + (1 if full else 0)
        rc = RC_LISTS[k % 3] if par == "scalar" else RC_LISTS[1 + k % 2]
        off, stride = (32, 64)[(k // 3 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        want, S, _ = _vref(box, drift, par)
        nl, qd, f = _forces(q, box, dtype, full, rc, par, off, stride)
        w = _virial(nl, qd, par)
        assert w.dtype == _torch().float64 and w.shape == (8,) and w.is_cuda
        w = w.cpu().numpy()
        print(box, drift, par, full, np.dtype(dtype).name, virial_ratio(w, want, S, dtype).round(3))
        check_virial(w, want, S, dtype)
        _check_energy(w, f, S, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,par", [("tilt", True, "typed32"), ("xyz", False, "scalar")])
def test_reproducible(box, drift, par, dtype):
    """Two calls return the same 64 bytes (also into another tensor, and from the enqueue variant); a half and a full
    build of the same input agree within twice the bound and on n_in."""
    q = _input(box, drift)
    want, S, _ = _vref(box, drift, par)
    got = {}
    for full in (False, True):
        nl, qd, _ = _forces(q, box, dtype, full, 3.4, par)
        a = _virial(nl, qd, par).cpu().numpy()
        b = _virial(nl, qd, par, out=_torch().empty(8, dtype=_torch().float64, device="cuda")).cpu().numpy()
        c = _virial(nl, qd, par, wait=False).cpu().numpy()
        assert a.tobytes() == b.tobytes() == c.tobytes() and len(a.tobytes()) == 64
        check_virial(a, want, S, dtype)
        got[full] = a
    assert np.all(np.abs(got[False][:7] - got[True][:7]) <= 2 * VIR_C * lj_unit(dtype) * S)
    assert got[False][7] == got[True][7]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box", ["xyz", "tilt"])
def test_one_type_is_the_scalar_path(box, full, dtype):
    """The by-type walk with a single type is the scalar walk, bit for bit: on one handle and one list, lj_virial and
    lj_virial_typed return the same 64 bytes and, after a full build, lj_forces and lj_forces_typed the same forces (the
    half list's atomics fix no order).  The parameters are not representable in float32, so both paths round them on the
    host; at rc = 3.6 rows are longer than 64 entries, so the 64-lane loop turns more than once and its last turn is
    ragged: lanes past the row's end stay in for the pick."""
    torch = _torch()
    eps, sig, rc = 0.7, 1.05, RC_LISTS[2]
    nl = _handle(box, dtype, full, rc)
    nl.Initialize(N)
    nl.set_type_cutoffs(np.zeros(N, dtype=np.int32), [[rc]])
    qd = torch.from_numpy(_input(box, False).astype(dtype)).cuda()
    nl.MakeNeighList(qd, N)
    nl.set_lj_type_params([[eps]], [[sig]], [[RCF]])
    rows = np.diff((nl.full_csr()[0] if full else nl.key_pointer()).cpu().numpy())
    assert rows.max() > 64 and (rows % 64 != 0).any()
    w = nl.lj_virial(qd, eps, sig, rc_force=RCF).cpu().numpy()
    assert np.isfinite(w).all() and w[7] > N
    assert w.tobytes() == nl.lj_virial_typed(qd).cpu().numpy().tobytes() and len(w.tobytes()) == 64
    if full:
        f = nl.lj_forces(qd, eps, sig, rc_force=RCF).cpu().numpy()
        assert np.isfinite(f).all() and f.tobytes() == nl.lj_forces_typed(qd).cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_more_rows_than_waves(full, dtype):
    """n = 10976 > 4 NBLK: the grid is capped, waves take a second row, the last turn is ragged."""
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    q, (want, S, _) = _big()
    n = len(q)
    assert n == 4 * N > 4 * NBLK and n % (4 * NBLK) != 0
    box6, _ = BIG_BOX
    nl = NeighListGPU(2.5, *box6[:3], dtype=_tdt(dtype), full_list=full, minimum_image=True)
    nl.Initialize(n)
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, n)
    w = nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF).cpu().numpy()
    f = nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF).cpu().numpy()
    print(full, np.dtype(dtype).name, virial_ratio(w, want, S, dtype).round(3))
    check_virial(w, want, S, dtype)
    _check_energy(w, f, S, dtype)
    if dtype == np.float64:
        _assert_sharp(S, "scalar", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box", ["open", "xyz", "tilt"])
def test_isolated_dimers(box, full, dtype):
    """One partner per particle, exact separations: the bound (sharp for fp32 too), n_in = the dimers inside rc_force; an
    input of dimers beyond the cut-off and coincident ones gives exactly 8 zeros."""
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    box6, mask = DIMER_BOXES[box]

    def run(q):
        nl = NeighListGPU(2.625, *box6[:3], dtype=_tdt(dtype), full_list=full, minimum_image=bool(mask), tilt=box6[3:])
        nl.Initialize(len(q))
        qd = torch.from_numpy(q.astype(dtype)).cuda()
        nl.MakeNeighList(qd, len(q))
        return nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF).cpu().numpy()

    for q, group in _dimer_inputs(box, dtype):
        assert np.array_equal(q.astype(dtype).astype(np.float64), q)
        want, S, _ = virial_reference(q, box6, mask, 1.0, 1.0, RCF)
        assert want[7] == (group < 2).sum() > 100
        _assert_sharp(S, "scalar", dtype)
        w = run(q)
        check_virial(w, want, S, dtype)
        out = np.repeat(group >= 2, 2)
        assert (group == 2).any() and (group == 3).any()
        assert np.array_equal(run(q[out]), np.zeros(8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,images", [("xyz", False), ("xyz", True), ("tilt", True)])
def test_reuse_within_the_skin(box, images, full, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants, scalar and typed; no extra build."""
    torch = _torch()
    q0, q1 = _input(box, False, True), _moved(box)
    for par in ("scalar", "typed3"):
        types, _, eps, sig, rcf = _par(par, 2.9)
        nl = _handle(box, dtype, full, 2.9, images=images)
        nl.set_skin(0.4)
        nl.Initialize(N)
        if types is not None:
            nl.set_type_cutoffs(types, _par(par, 2.9)[1])
            nl.set_lj_type_params(eps, sig, rcf)
        qd = torch.from_numpy(q0.astype(dtype)).cuda()
        nl.update(qd, sync=True)
        builds = nl.update_stats()[1]
        qd.copy_(torch.from_numpy(q1.astype(dtype)))
        nl.update(qd)
        w = _virial(nl, qd, par, wait=False)
        torch.cuda.synchronize()
        assert nl.update_stats()[1] == builds
        want, S, _ = _moved_vref(box, par)
        check_virial(w.cpu().numpy(), want, S, dtype)


@pytest.mark.gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: 8 NaN, NL_ERR_CAPACITY at synchronize (a
    status code); after the synchronous repeat the result is finite."""
    from md_neighbor_list_amd import NeighListGPU, inputs
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = NeighListGPU(3.3, *box, dtype=torch.float32)
    nl.set_skin(0.4)
    nl.Initialize(len(q))
    nl.set_capacity(1000)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd)
    w = nl.lj_virial(qd, wait=False)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert torch.isnan(w).all() and w.shape == (8,)
    nl.update(qd)  # the host has seen the failure: builds (and fails) again
    with pytest.raises(NLError):
        nl.synchronize()
    nl.update(qd, sync=True)  # grows the list
    w = nl.lj_virial(qd, wait=False)
    assert torch.isfinite(w).all() and w[7] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_captured(full, dtype):
    """One graph holds the copy of the positions, the update and the virial; replayed at three position sets.  A first
    virial call inside a capture, on a handle whose scratch does not exist yet, is NL_ERR_STATE."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()
    sets = [(_input("xyz", False, True), _vref("xyz", False, "scalar", True)), (_moved("xyz"), _moved_vref("xyz", "scalar")),
            (_moved("xyz", 0.03, 22), _moved_vref("xyz", "scalar", 22))]
    nl = _handle("xyz", dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    src = torch.from_numpy(sets[0][0].astype(dtype)).cuda()
    qd = src.clone()
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    nl.update(qd, sync=True)
    fresh = _handle("xyz", dtype, full, 2.9)
    fresh.Initialize(N)
    fresh.MakeNeighList(qd, N)
    nl.update(qd)
    nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)  # once before the capture: the scratch exists
    nl.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)
        with pytest.raises(NLError) as e:
            fresh.lj_virial(qd, rc_force=RCF, wait=False)
    assert e.value.code == NL_ERR_STATE
    for q, (want, S, _) in sets:
        src.copy_(torch.from_numpy(q.astype(dtype)))
        wd.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        check_virial(wd.cpu().numpy(), want, S, dtype)
    check_virial(fresh.lj_virial(qd, rc_force=RCF).cpu().numpy(), *sets[2][1][:2], dtype)  # (outside: it allocates and runs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_exclusions(full, dtype):
    """The bonded neighbours are absent from the totals; the unfiltered reference is refused under the fp64 bound."""
    want, S, _ = _excluded_vref()
    nl, qd, f = _forces(_input("xyz", False), "xyz", dtype, full, 2.5, "scalar", exclusions=_bonds())
    w = nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF).cpu().numpy()
    check_virial(w, want, S, dtype)
    _check_energy(w, f, S, dtype)
    assert want[7] == _vref("xyz", False, "scalar")[0][7] - len(_bonds())
    if dtype == np.float64:
        with pytest.raises(AssertionError):
            check_virial(w, _vref("xyz", False, "scalar")[0], S, dtype, count=False)


@pytest.mark.gpu
def test_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    d = C.c_double
    assert lib.nl_lj_virial_enqueue(nl._h, qd.data_ptr(), 4, d(1), d(1), d(2.5), out.data_ptr(), None) == NL_ERR_STATE  # no list yet
    nl.MakeNeighList(qd, N)
    assert lib.nl_lj_virial(nl._h, qd.data_ptr(), 4, d(1), d(1), d(2.5), None, None) == NL_ERR_ARG
    assert lib.nl_lj_virial_enqueue(nl._h, qd.data_ptr(), 4, d(1), d(1), d(2.5), None, None) == NL_ERR_ARG
    assert lib.nl_lj_virial_typed(nl._h, qd.data_ptr(), 4, None, None) == NL_ERR_ARG
    assert lib.nl_lj_virial_typed_enqueue(nl._h, qd.data_ptr(), 4, None, None) == NL_ERR_ARG
    assert lib.nl_lj_virial(nl._h, None, 4, d(1), d(1), d(2.5), out.data_ptr(), None) == NL_ERR_ARG
    for stride in (0, 2, 5):
        assert lib.nl_lj_virial(nl._h, qd.data_ptr(), stride, d(1), d(1), d(2.5), out.data_ptr(), None) == NL_ERR_ARG
        assert lib.nl_lj_virial_typed(nl._h, qd.data_ptr(), stride, out.data_ptr(), None) == NL_ERR_ARG
    for bad in (dict(rc_force=2.95), dict(rc_force=0.0), dict(sigma=0.0), dict(rc_force=2.6, wait=False)):  # rc = 2.9, skin = 0.4
        with pytest.raises(NLError) as e:
            nl.lj_virial(qd, **bad)
        assert e.value.code == NL_ERR_ARG, bad
    nl.lj_virial(qd, rc_force=2.9)
    nl.lj_virial(qd, rc_force=2.5, wait=False)
    for wait in (True, False):  # typed calls without a table
        with pytest.raises(NLError) as e:
            nl.lj_virial_typed(qd, wait=wait)
        assert e.value.code == NL_ERR_STATE
    with pytest.raises(TypeError):
        nl.lj_virial(qd, out=torch.empty(8, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        nl.lj_virial(qd, out=torch.empty(7, dtype=torch.float64, device="cuda"))
    # a type table without parameters
    types, rc_ab, eps, sig, rcf = _par("typed3", 2.9)
    nl.set_type_cutoffs(types, rc_ab)
    nl.MakeNeighList(qd, N)
    with pytest.raises(NLError) as e:
        nl.lj_virial_typed(qd)
    assert e.value.code == NL_ERR_STATE
    nl.set_lj_type_params(eps, sig, rcf)
    assert torch.isfinite(nl.lj_virial_typed(qd)).all()
    nl.lj_virial_typed(qd, wait=False)  # rc_force_ab = 2.5 sigma_ab / 1.1 reaches 2.5 = rc - skin ...
    nl.set_skin(0.6)  # ... and lies beyond it with a wider skin
    with pytest.raises(NLError) as e:
        nl.lj_virial_typed(qd, wait=False)
    assert e.value.code == NL_ERR_ARG
    # a slab build has no totals
    slab = _handle("open", np.float32, False, 2.9)
    mz = slab.mesh_size[2]
    edge = LJ_L / mz
    inner = q[(q[:, 2] > edge + 0.2) & (q[:, 2] < (mz - 1) * edge - 0.2)]  # the layers 1 .. mz - 2, their ghost layers empty
    assert mz == 5 and 1000 < len(inner) < N
    slab.Initialize(len(inner))
    qs = torch.from_numpy(inner.astype(np.float32)).cuda()
    slab.MakeNeighListSlab(qs, None, len(inner), 1, mz - 1)
    assert slab.half_number_of_pairs() > 0
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            slab.lj_virial(qs, rc_force=2.5, wait=wait)
        assert e.value.code == NL_ERR_STATE
    # n == 0
    empty = _handle("open", np.float32, False, 2.9)
    empty.Initialize(16)
    empty.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    out.fill_(7.0)  # (an empty tensor has no address to pass: the positions are not read)
    assert lib.nl_lj_virial(empty._h, qd.data_ptr(), 4, d(1), d(1), d(2.5), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.zeros(8))

"""The Lennard-Jones consumer (nl_lj_forces, nl_lj_forces_typed and their enqueue variants) against an O(N^2) float64 sum,
with an error bound per particle and per component.

Contract tested (include/nl_hip.h, nl_lj_forces):
  * |got - want| <= c u S for every particle and each of fx, fy, fz, pe on its own: want the float64 sum of tests.util
    lj_reference (no list, the library's or the oracle's), S the uncancelled sum of that component's pair terms, u = 2^-24
    (fp32) or 2^-53 (fp64);
  * positions up to one box length outside the box (drifted, never wrapped), orthogonal and tilted boxes, every mask;
  * rc_force exact for every pair further than 64 ulp (in r) from it: full force below, exactly 0 above.

c = LJ_C = 51.2 for both dtypes.  It is not fitted to the kernel: it is 4 x the largest |emulated - want| / (u S) = 12.80 that
a float32 numpy emulation of lj_pair and lj_image reaches (one rounding per operation, no FMA, every particle's terms summed
in a random order) over the inputs of EMULATED, three summation orders each; test_emulation_gives_c recomputes that maximum.
The factor 4 covers the GPU's other summation tree and the rounding of 4 eps, sigma^2, rc_force^2 and the box on the host.
The bound is sharp (test_bound_is_sharp): on every input c u S stays below a quarter of what one pair at rc_force gives a
component, so dropping any single pair, the weakest included, fails the check; test_wrong_results_are_rejected shows it
on six deliberately wrong results.

The inputs (tests.util lj_lattice): a 14^3 simple-cubic lattice, a = 1.125, L = 15.75 (exact in float32), sites
(k + 1/2) a jittered by +-0.10 per axis, n = 2744, closest pair 0.925; tilts of whole lattice spacings; drifted: plus a whole
lattice vector from {-1, 0, +1}^3 per particle.  Both dtypes get the same float32 values, so one reference serves both.
"""
import functools

import numpy as np
import pytest

from tests.consumer_util import CASES, EMULATED, N, PARS, RC_LISTS, RCF, _bonds, _dimers, _handle, _torch
from tests.consumer_util import _lj_forces as _forces
from tests.consumer_util import _lj_input as _input
from tests.consumer_util import _lj_moved as _moved
from tests.consumer_util import _lj_moved_pairs as _moved_pairs
from tests.consumer_util import _lj_pairs as _pairs
from tests.consumer_util import _lj_par as _par
from tests.util import (LJ_A, LJ_BOXES, LJ_C, LJ_L, check_lj, lj_band_particles, lj_drift, lj_emulate, lj_fold, lj_fractional, lj_pairs,
                        lj_ratio, lj_reference, lj_unit)

EMULATED_MAX = 12.80  # the largest ratio of test_emulation_gives_c (force columns; energy 5.3)


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _ref(box, drift, par, shift=False):
    box6, mask = LJ_BOXES[box]
    types, _, eps, sig, rcf = _par(par)
    return lj_reference(_input(box, drift, shift), box6, mask, eps, sig, rcf, types=types, pairs=_pairs(box, drift, shift))


def _single(par):
    """(|F(rc_force)| of the weakest pair a particle can have, its |U| / 2), per particle: what dropping one pair at the
    cut-off takes from a component at the least."""
    types, rc, eps, sig, rcf = _par(par)
    eps, sig, rcf = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (eps, sig, rcf))
    live = rcf > 0
    r = np.where(live, rcf, 1.0)
    s6 = (sig / r) ** 6
    F = np.where(live, np.abs(24.0 * eps * (2.0 * s6 * s6 - s6) / r), np.inf).min(axis=1)
    U = np.where(live, np.abs(2.0 * eps * (s6 * s6 - s6)), np.inf).min(axis=1)
    t = np.zeros(N, dtype=np.int64) if types is None else types
    return F[t], U[t]


def _assert_sharp(S, par, c=LJ_C):
    F, U = _single(par)
    u = lj_unit(np.float32)
    assert np.all(c * u * S[:, :3].max(axis=1) <= 0.25 * F / np.sqrt(3.0)), (c * u * S[:, :3].max(axis=1) / F).max()
    assert np.all(c * u * S[:, 3] <= 0.25 * U), (c * u * S[:, 3] / U).max()


# ------------------------------------------------------------------------------------------------- CPU: the checker
def test_single_pair_values():
    F, U = _single("scalar")
    assert abs(F[0] - 0.039) < 5e-4 and abs(U[0] - 0.00816) < 5e-6
    assert abs(LJ_L - 15.75) == 0 and np.float32(LJ_L) == LJ_L and np.float32(LJ_A) == LJ_A


def test_reference_is_the_gradient_of_its_energy():
    """lj_reference's forces against the central difference of its own total energy, tilted and periodic."""
    rng = np.random.default_rng(3)
    m, a = 5, 1.125
    box6, mask = (m * a, m * a, m * a, a, -a, 2 * a), 7
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (g + 0.5) * a + rng.uniform(-0.1, 0.1, size=g.shape)
    rcf, h = 2.2, 1e-5
    types = rng.integers(0, 2, size=len(q))
    eps, sig = np.array([[1.0, 1.7], [1.7, 0.6]]), np.array([[1.0, 0.95], [0.95, 1.05]])
    near = set(lj_band_particles(q, box6, mask, (rcf,), 1e-3).tolist())  # (a pair crossing the cut-off is a jump in E)
    want, S = lj_reference(q, box6, mask, eps, sig, rcf, types=types)
    picked = [i for i in range(len(q)) if i not in near][:4]
    assert len(picked) == 4
    for i in picked:
        for c in range(3):
            e = []
            for sgn in (1.0, -1.0):
                p = q.copy()
                p[i, c] += sgn * h
                e.append(lj_reference(p, box6, mask, eps, sig, rcf, types=types)[0][:, 3].sum())
            fd = -(e[0] - e[1]) / (2 * h)
            assert abs(fd - want[i, c]) <= 1e-6 * S[i, c], (i, c, fd, want[i, c])
    assert np.abs(want[:, :3].sum(axis=0)).max() <= 1e-12 * S[:, :3].sum()  # Newton's third law in the reference


def test_emulation_gives_c():
    """c = 4 x the largest |emulated - want| / (u S) of a float32 emulation of the kernel's arithmetic (never the kernel)."""
    worst = np.zeros(4)
    for box, drift, par in EMULATED:
        box6, mask = LJ_BOXES[box]
        types, _, eps, sig, rcf = _par(par)
        want, S = _ref(box, drift, par)
        I, J, d, raw = _pairs(box, drift)
        near = (d * d).sum(axis=1) < 2.51 ** 2  # (the rest is skipped by the cut-off test: exactly 0)
        for order in range(3):
            f = lj_emulate(_input(box, drift), box6, mask, eps, sig, rcf, np.float32, np.random.default_rng(100 + order),
                           (I[near], J[near]), types=types)
            r = lj_ratio(f, want, S, np.float32).max(axis=0)
            print(box, drift, par, order, r.round(2))
            worst = np.maximum(worst, r)
    print("largest ratio per column", worst)
    assert worst.max() <= EMULATED_MAX <= LJ_C / 4


def test_bound_is_sharp():
    """On every input c u S <= 1/4 |F(rc_force)| / sqrt(3) and <= 1/4 |U(rc_force) / 2|, per particle: the allowance of
    fp32 is a quarter of the weakest single pair, so no pair can go missing unnoticed."""
    seen = 0
    for box, drift in CASES:
        for par in PARS:
            _assert_sharp(_ref(box, drift, par)[1], par)
            seen += 1
    for box in ("xyz", "tilt"):
        q = _moved(box)
        box6, mask = LJ_BOXES[box]
        for par in ("scalar", "typed3"):
            types, _, eps, sig, rcf = _par(par)
            _assert_sharp(lj_reference(q, box6, mask, eps, sig, rcf, types=types, pairs=_moved_pairs(box))[1], par)
    _assert_sharp(_excluded_ref()[1], "scalar")
    assert seen == 27
    S = _ref("xyz", False, "scalar")[1]
    assert 150 < S[:, :3].max() < 250 and S[:, 3].max() < 30


def _single_fold(d, box6, mask):
    """The one half-box test per axis that lj_image had: wrong beyond 1.5 L."""
    for a in range(3):
        if mask >> a & 1:
            L = box6[a]
            d[:, a] = np.where(d[:, a] > 0.5 * L, d[:, a] - L, np.where(d[:, a] < -0.5 * L, d[:, a] + L, d[:, a]))
    return d


def _term(d, eps=1.0, sig=1.0):
    r2 = (d * d).sum(axis=1)
    s6 = (sig * sig / r2) ** 3
    return np.concatenate([(24.0 * eps * (2.0 * s6 * s6 - s6) / r2)[:, None] * d, (2.0 * eps * (s6 * s6 - s6))[:, None]], axis=1)


def test_wrong_results_are_rejected():
    """check_lj on float64 results with one deliberate defect each, under the fp32 bound: all six are refused."""
    box6, mask = LJ_BOXES["xyz"]
    q, (I, J, d, raw) = _input("xyz", False), _pairs("xyz", False)
    want, S = _ref("xyz", False, "scalar")
    check_lj(want, want, S, np.float32)
    wrong = {}
    # every row's last entry dropped (rows of the full list at rc = rc_force, partners ascending)
    r2 = (d * d).sum(axis=1)
    inn = r2 < RCF * RCF
    Ii, Ji, di = I[inn], J[inn], d[inn]
    order = np.lexsort((Ji, Ii))
    last = order[np.r_[np.flatnonzero(np.diff(Ii[order])), len(order) - 1]]
    w = want.copy()
    np.subtract.at(w, Ii[last], _term(di[last]))
    wrong["last entry of every row"] = w
    wrong["pairs beyond 0.9 rc_force"] = lj_reference(q, box6, mask, 1.0, 1.0, 0.9 * RCF, pairs=(I, J, d, raw))[0]
    wrong["cut at the list's rc"] = lj_reference(q, box6, mask, 1.0, 1.0, 3.4, pairs=(I, J, d, raw))[0]
    # one face-crossing pair at its raw coordinates: beyond rc_force there, so it leaves both particles
    k = int(np.flatnonzero(inn & (np.abs(raw).max(axis=1) > 0.5 * LJ_L))[0])
    w = want.copy()
    w[I[k]] -= _term(d[k:k + 1])[0]
    w[J[k]] -= _term(-d[k:k + 1])[0]
    wrong["a face-crossing pair at raw coordinates"] = w
    for name, w in wrong.items():
        with pytest.raises(AssertionError):
            check_lj(w, want, S, np.float32)
        assert name
    # the single half-box fold, on the drifted input
    qd = _input("xyz", True)
    wd, Sd = _ref("xyz", True, "scalar")
    w = lj_reference(qd, box6, mask, 1.0, 1.0, RCF, pairs=lj_pairs(qd, box6, mask, RCF, fold=_single_fold))[0]
    with pytest.raises(AssertionError):
        check_lj(w, wd, Sd, np.float32)
    # eps_ab read as eps_ba, from a matrix made asymmetric for the purpose
    types, _, eps, sig, rcf = _par("typed32")
    asym = eps * (1.0 + 0.02 * np.triu(np.ones_like(eps), 1))
    wa, Sa = lj_reference(q, box6, mask, asym, sig, rcf, types=types, pairs=(I, J, d, raw))
    w = lj_reference(q, box6, mask, asym.T, sig, rcf, types=types, pairs=(I, J, d, raw))[0]
    with pytest.raises(AssertionError):
        check_lj(w, wa, Sa, np.float32)


def test_checker_reports_the_worst_particle():
    want, S = _ref("xyz", False, "scalar")
    w = want.copy()
    w[77, 1] += 10 * LJ_C * lj_unit(np.float32) * S[77, 1]
    with pytest.raises(AssertionError, match=r"particle 77, column y"):
        check_lj(w, want, S, np.float32)
    w = want.copy()
    w[5, 3] = np.nan
    with pytest.raises(AssertionError, match=r"particle 5, column e"):
        check_lj(w, want, S, np.float64)


def test_inputs():
    for box, drift in CASES:
        box6, mask = LJ_BOXES[box]
        q = _input(box, drift)
        assert len(q) == N == 2744 and np.array_equal(q[:, :3], q[:, :3].astype(np.float32))
        I, J, d, raw = _pairs(box, drift)
        r = np.sqrt((d * d).sum(axis=1))
        assert 0.92 < r.min() < 0.95
        if drift:
            for a in range(3):
                if mask >> a & 1:  # both signs, and listed pairs with a raw separation beyond 1.5 L on the axis
                    assert (q[:, a] < 0).any() and (q[:, a] >= box6[a]).any()
                    assert (np.abs(raw[r < RCF, a]) > 1.5 * box6[a]).any()
    for name in PARS[1:]:
        types, rc, eps, sig, rcf = _par(name)
        nt = len(eps)
        I, J = _pairs("xyz", False)[:2]
        assert set(types.tolist()) == set(range(nt))
        assert len(set((types[I] * nt + types[J]).tolist())) == nt * nt  # every ordered pair of types is a (row, partner)
        assert eps.max() / eps.min() > 49.9 and sig.min() == 0.9 and abs(sig.max() - 1.1) < 1e-12
        assert rc[0, nt - 1] == 0 and len(np.unique(rcf)) > nt


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _check_sums(got, want, S, dtype):
    """Total force within c u sum_i S_i of zero's float64 value, total energy within the same kind of bound."""
    u = lj_unit(dtype)
    g = got.astype(np.float64).sum(axis=0)
    assert np.all(np.abs(g - want.sum(axis=0)) <= LJ_C * u * S.sum(axis=0)), (g, want.sum(axis=0))


# -------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, full, dtype):
    """Every box, mask and position state x scalar and typed parameters x list kind x dtype; the list cut-off (2.5, 3.4,
    3.6: one, two and three turns of lj_row's lane loop), the offset width and q_stride rotate through the cases."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, par in enumerate(PARS):
        k = case + p + (1 if full else 0)
        rc = RC_LISTS[k % 3] if par == "scalar" else RC_LISTS[1 + k % 2]
        off, stride = (32, 64)[(k // 3 + p) % 2], (4, 3)[(k + (dtype == np.float64)) % 2]
        want, S = _ref(box, drift, par)
        nl, _, got = _forces(q, box, dtype, full, rc, par, off, stride)
        if full and LJ_BOXES[box][1] == 7 and rc > RCF:  # ~115 and ~137 entries per row: two and three turns of 64 lanes
            cnt = nl.number_of_partners().cpu().numpy()[:N]
            types = _par(par)[0]
            if types is not None:  # (the rows of the two types whose pair has rc_ab = 0 are shorter)
                cnt = cnt[(types != 0) & (types != types.max())]
            lo, hi = {3.4: (105, 125), 3.6: (128, 147)}[rc]
            assert cnt.min() > 64 and lo < np.median(cnt) < hi, (cnt.min(), np.median(cnt), cnt.max())
        check_lj(got, want, S, dtype)
        _check_sums(got, want, S, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
def test_offsets_strides_and_type_counts(full, dtype):
    """The full cross of offset width x q_stride x parameters on the drifted tilted lattice."""
    want = {par: _ref("tilt", True, par) for par in PARS}
    for off in (32, 64):
        for stride in (3, 4):
            for par in PARS:
                _, _, got = _forces(_input("tilt", True), "tilt", dtype, full, 3.4, par, off, stride)
                check_lj(got, *want[par], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box", ["open", "xyz", "tilt"])
def test_isolated_dimers(box, full, dtype):
    """One partner per particle: the pair's force and energy within c u of their magnitude, exactly 0 beyond rc_force and for
    coincident partners, F_i == -F_j bit for bit; in the box, across one, two and three faces, and with the partners moved
    apart by whole lattice vectors (some to opposite sides outside the box)."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    L, g = 63.0, 10.5
    box6, mask = {"open": ((L, L, L, 0.0, 0.0, 0.0), 0), "xyz": ((L, L, L, 0.0, 0.0, 0.0), 7),
                  "tilt": ((L, L, L, g, -g, 2 * g), 7)}[box]
    base, group, inner = _dimers(dtype, box6, mask)
    n = len(base)
    shifts = np.random.default_rng(9).integers(-1, 2, size=(n, 3))
    first, second = 2 * inner[:20], 2 * inner[:20] + 1
    shifts[first], shifts[second] = (-1, 0, 1), (1, 0, -1)  # both partners outside, on opposite sides
    for q in ([base] if not mask else [base, lj_drift(base, 0, (box6, mask), k=shifts)]):
        assert np.array_equal(q.astype(dtype).astype(np.float64), q)
        if q is not base:
            assert (q[first, 0] < 0).all() and (q[second, 0] >= L).all()
        want, S = lj_reference(q, box6, mask, 1.0, 1.0, RCF)
        assert np.all(S[np.repeat(group >= 2, 2)] == 0) and np.all(S[np.repeat(group < 2, 2), 3] > 0)
        assert np.allclose(want[np.repeat(group == 1, 2), 3], -0.00816, atol=1e-5)  # half of -0.016 eps each
        nl = NeighListGPU(2.625, L, L, L, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                          minimum_image=bool(mask), tilt=box6[3:])
        nl.Initialize(n)
        qd = torch.from_numpy(q.astype(dtype)).cuda()
        nl.MakeNeighList(qd, n)
        assert (group < 3).sum() <= nl.half_number_of_pairs() <= n // 2  # every molecule is listed; nothing else
        got = nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF).cpu().numpy()
        assert not np.isnan(got).any()
        check_lj(got, want, S, dtype)
        assert np.all(got[np.repeat(group >= 2, 2)] == 0)
        assert np.array_equal(got[0::2, :3], -got[1::2, :3]) and np.array_equal(got[0::2, 3], got[1::2, 3])


def test_moved_input():
    for box in ("xyz", "tilt"):
        box6, mask = LJ_BOXES[box]
        q0, q1 = _input(box, False, True), _moved(box)
        assert np.abs(q1 - q0).max() <= 0.03 + 1e-6
        l0, l1 = lj_fractional(q0[:, :3], box6), lj_fractional(q1[:, :3], box6)
        assert (l0 > -1e-6).all() and (l0 < 1 + 1e-6).all()
        # out through the faces (the tilted x and y faces cut between the lattice planes: few particles are near them):
        # rule (c) without the fold keeps the list, the positions stay unwrapped
        out = (l1 < -1e-4).any(axis=0) & (l1 > 1 + 1e-4).any(axis=0)
        assert out[2] and (out.all() or box == "tilt")
        I, J, d, _ = _pairs(box, False, True)
        before = np.sqrt((d * d).sum(axis=1))
        after = np.sqrt((lj_fold(q1[I, :3] - q1[J, :3], box6, mask) ** 2).sum(axis=1))
        assert ((before < RCF) & (after > RCF)).any() and ((before > RCF) & (after < RCF)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,images", [("xyz", False), ("xyz", True), ("tilt", True)])
def test_reuse_within_the_skin(box, images, full, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants: scalar and typed, with particles
    that have left through a face (pair images on: rule (c) does not fold, positions stay unwrapped)."""
    torch = _torch()
    box6, mask = LJ_BOXES[box]
    q0, q1 = _input(box, False, True), _moved(box)
    for par in ("scalar", "typed3"):
        types, _, eps, sig, rcf = _par(par, 2.9)
        nl = _handle(box, dtype, full, 2.9, images=images)
        nl.set_skin(0.4)
        nl.Initialize(N)
        if types is not None:
            nl.set_type_cutoffs(types, _par(par, 2.9)[1])
        qd = torch.from_numpy(q0.astype(dtype)).cuda()
        nl.update(qd, sync=True)
        builds = nl.update_stats()[1]
        qd.copy_(torch.from_numpy(q1.astype(dtype)))
        nl.update(qd)
        if types is not None:
            nl.set_lj_type_params(eps, sig, rcf)
            f = nl.lj_forces_typed(qd, wait=False)
        else:
            f = nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF, wait=False)
        torch.cuda.synchronize()
        # (without the images the folded rule keeps the list as well: every move is below skin / 2)
        assert nl.update_stats()[1] == builds
        want, S = lj_reference(q1, box6, mask, eps, sig, rcf, types=types, pairs=_moved_pairs(box))
        check_lj(f.cpu().numpy(), want, S, dtype)


@functools.lru_cache(maxsize=None)
def _excluded_ref():
    box6, mask = LJ_BOXES["xyz"]
    return lj_reference(_input("xyz", False), box6, mask, 1.0, 1.0, RCF, exclusions=_bonds(), pairs=_pairs("xyz", False))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
def test_exclusions(full, dtype):
    """Bonded neighbours, the strongest pairs of the system, are absent from the forces; the unfiltered sum is refused."""
    want, S = _excluded_ref()
    _, _, got = _forces(_input("xyz", False), "xyz", dtype, full, 2.5, "scalar", exclusions=_bonds())
    check_lj(got, want, S, dtype)
    with pytest.raises(AssertionError):
        check_lj(got, _ref("xyz", False, "scalar")[0], S, dtype)

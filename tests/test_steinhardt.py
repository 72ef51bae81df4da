"""Steinhardt order parameters from the list (nl_set_steinhardt, nl_steinhardt).

The contract is this family's own (the Consumer of tests.consumer_contract assumes forces plus totals): N_b exact and q_lm, q_l,
w_l and the averaged forms within STEIN_C u S of an O(N^2) float64 reference with independent harmonics (tests.util_steinhardt),
on inputs none of whose pairs lies within 2^-17 (relative, r^2) of r_max^2 -- so no particle is left out of any comparison.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from md_neighbor_list_amd import steinhardt as st
from tests import util_steinhardt as us
from tests.consumer_util import CASES, DTYPES, N, SEED, _bonds, _handle, _tdt, _torch
from tests.util import LJ_BOXES, lj_band_particles, lj_drift, lj_lattice, lj_pairs, lj_type_params

gpu = pytest.mark.gpu
BAND = 2.0 ** -17
R_NEAR, R_FAR = 1.45, 2.0   # the two neighbour ranges of the lattice inputs
RC = {R_NEAR: 1.5, R_FAR: 2.1}  # the list cut-offs they are read from


# ---------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def _input(box, drift, r_max=R_NEAR):
    """The 14^3 jittered lattice with no pair in the band of r_max, [n, 4] float64 holding float32 values."""
    if drift:
        q = lj_drift(_input(box, False, r_max), SEED + 1, box)
    else:
        q = lj_lattice(SEED, box, cuts=(r_max,))
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _pairs(box, drift, r_max=R_NEAR):
    box6, mask = LJ_BOXES[box]
    p = lj_pairs(_input(box, drift, r_max), box6, mask, r_max * (1 + 2.0 ** -12))
    assert not len(lj_band_particles(None, box6, mask, (r_max,), BAND, pairs=p)), "a pair in the band of r_max"
    return p


@functools.lru_cache(maxsize=None)
def _ref(box, drift, l, r_max=R_NEAR):
    box6, mask = LJ_BOXES[box]
    return us.reference(_input(box, drift, r_max), box6, mask, l, r_max, pairs=_pairs(box, drift, r_max))


@functools.lru_cache(maxsize=None)
def _moved(box="xyz", step=0.03, seed=21, r_max=R_NEAR):
    """The lattice with every particle moved by up to `step` per axis (far below skin / 2), none ending in the band."""
    box6, mask = LJ_BOXES[box]
    q0 = _input(box, False, r_max)
    rng = np.random.default_rng(seed)
    q, todo = q0.copy(), np.arange(N)
    for _ in range(20):
        q[todo, :3] = (q0[todo, :3] + rng.uniform(-step, step, size=(len(todo), 3))).astype(np.float32)
        todo = lj_band_particles(q, box6, mask, (r_max,), 2.0 ** -15, rows=todo)
        if not len(todo):
            break
    assert not len(todo)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _moved_ref(l, box="xyz"):
    box6, mask = LJ_BOXES[box]
    return us.reference(_moved(box), box6, mask, l, R_NEAR)


def _band_free_uniform(n, L, r_max, seed):
    """n uniform particles in a periodic cube of edge L, float32 values; particles with a partner in the band of r_max are
    drawn again (as lj_lattice does it)."""
    rng = np.random.default_rng(seed)
    box6, mask = (L, L, L, 0.0, 0.0, 0.0), 7
    q = np.zeros((n, 4))
    q[:, :3] = rng.uniform(0.0, 0.999 * L, size=(n, 3)).astype(np.float32)
    bad = None
    for _ in range(20):
        bad = lj_band_particles(q, box6, mask, (r_max,), 2.0 ** -15, rows=bad)
        if not len(bad):
            return q, box6, mask
        q[bad, :3] = rng.uniform(0.0, 0.999 * L, size=(len(bad), 3)).astype(np.float32)
    raise AssertionError("pairs stay in the band of r_max")


@functools.lru_cache(maxsize=None)
def _long_rows():
    """4096 uniform particles at density 1, r_max = 3.0: about 113 neighbours a row.  (q, box6, mask, reference at l = 6)"""
    q, box6, mask = _band_free_uniform(4096, 16.0, 3.0, 31)
    pairs = lj_pairs(q, box6, mask, 3.0 * (1 + 2.0 ** -12))
    assert not len(lj_band_particles(None, box6, mask, (3.0,), BAND, pairs=pairs))
    q.setflags(write=False)
    return q, box6, mask, us.reference(q, box6, mask, 6, 3.0, pairs=pairs)


@functools.lru_cache(maxsize=None)
def _dimers():
    """500 dimers of bond length 1 on a 8^3 grid of spacing 3 (L = 24), random orientations, the first three along x, y, z."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*(np.arange(8),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:500]
    u = rng.normal(size=(500, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    u[:3] = np.eye(3)
    q = np.zeros((1000, 4))
    q[0::2, :3] = (g + 0.5) * 3.0 - 0.5 * u  # (atoms of different dimers are 2 apart at least)
    q[1::2, :3] = (g + 0.5) * 3.0 + 0.5 * u
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q, (24.0, 24.0, 24.0, 0.0, 0.0, 0.0), 7


@functools.lru_cache(maxsize=None)
def _dimer_pairs():
    q, box6, mask = _dimers()
    return lj_pairs(q, box6, mask, 1.3)


def _ideal_shell(name):
    """The bond vectors of an ideal first shell (bcc14: first and second)."""
    import itertools

    def perm(v):  # every permutation of v with every choice of signs, once each
        return {tuple(float(s * c) + 0.0 for s, c in zip(sg, p)) for p in itertools.permutations(v) for sg in itertools.product((-1, 1), repeat=3)}

    s3 = np.sqrt(3.0)
    if name == "fcc":
        return np.array(sorted(perm((1, 1, 0))), dtype=np.float64)
    if name == "bcc":
        return np.array(sorted(perm((1, 1, 1))), dtype=np.float64)
    if name == "bcc14":
        return np.array(sorted(perm((1, 1, 1)) | perm((2, 0, 0))), dtype=np.float64)
    if name == "sc":
        return np.array(sorted(perm((1, 0, 0))), dtype=np.float64)
    ring = [(np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0) for k in range(6)]
    c = np.sqrt(2.0 / 3.0)
    up = [(np.cos(a) / s3, np.sin(a) / s3, c) for a in (np.pi / 6, np.pi / 6 + 2 * np.pi / 3, np.pi / 6 + 4 * np.pi / 3)]
    return np.array(ring + up + [(x, y, -z) for x, y, z in up])


def _shell_values(v, l):
    """(q_l, w_l) of the bond vectors v in float64, by the reference's formulas."""
    u = v / np.linalg.norm(v, axis=1)[:, None]
    qlm = us.ylm(l, u[:, 0], u[:, 1], u[:, 2]).mean(axis=0)[None, :]
    ql, wl, _, _ = us._columns(us.full_qlm(qlm), np.zeros(1), l)
    return float(ql[0]), float(wl[0])


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_reference_harmonics_match_scipy():
    rng = np.random.default_rng(2)
    u = rng.normal(size=(400, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    u[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    for l in range(1, st.MAX_L + 1):
        Y = us.ylm(l, u[:, 0], u[:, 1], u[:, 2])
        for m in range(l + 1):
            assert np.abs(Y[:, m] - us.scipy_ylm(l, m, u[:, 0], u[:, 1], u[:, 2])).max() < 1e-13, (l, m)


def test_reference_reproduces_the_known_answers():
    """The table of CRYSTALS to its printed six decimals, and the values with a closed form to 1e-9."""
    for name, want in st.CRYSTALS.items():
        v = _ideal_shell(name)
        assert len(v) == {"fcc": 12, "hcp": 12, "bcc": 8, "bcc14": 14, "sc": 6}[name]
        q4, w4 = _shell_values(v, 4)
        q6, w6 = _shell_values(v, 6)
        assert np.allclose([q4, q6, w4, w6], want, rtol=0, atol=5.1e-7), (name, q4, q6, w4, w6)
    exact = {("fcc", 4): np.sqrt(7 / 192), ("fcc", 6): np.sqrt(169 / 512), ("hcp", 4): 7 / 72, ("bcc", 4): np.sqrt(7 / 27),
             ("bcc", 6): np.sqrt(32 / 81), ("sc", 4): np.sqrt(7 / 12), ("sc", 6): np.sqrt(1 / 8)}
    for (name, l), want in exact.items():
        assert abs(_shell_values(_ideal_shell(name), l)[0] - want) < 1e-9, (name, l)
    assert abs(_shell_values(_ideal_shell("hcp"), 4)[1] - np.sqrt(18 / 1001)) < 1e-9
    assert abs(_shell_values(_ideal_shell("fcc"), 12)[0] - 0.600083) < 5.1e-7
    for l in range(1, st.MAX_L + 1):  # a single bond: q_l = 1 by the sum rule, w_l = (l l l; 0 0 0)
        ql, wl = _shell_values(np.array([[0.3, -0.5, 0.7]]), l)
        assert abs(ql - 1) < 1e-12 and abs(wl - st.wigner3j_table(l)[l, l]) < 1e-12
    assert abs(st.wigner3j_table(4)[4, 4] - np.sqrt(18 / 1001)) < 1e-15 and st.wigner3j_table(5)[5, 5] == 0


def test_wigner3j_table_equals_sympy():
    pytest.importorskip("sympy")
    from sympy import N as evalf
    from sympy.physics.wigner import wigner_3j

    for l in range(1, st.MAX_L + 1):
        w = st.wigner3j_table(l)
        assert w.shape == (2 * l + 1, 2 * l + 1)
        for m1 in range(-l, l + 1):
            for m2 in range(-l, l + 1):
                want = float(evalf(wigner_3j(l, l, l, m1, m2, -m1 - m2), 30)) if abs(m1 + m2) <= l else 0.0
                assert abs(w[m1 + l, m2 + l] - want) <= 2.0 ** -52 * abs(want), (l, m1, m2)


EMULATED = [("xyz", False, 4, R_NEAR), ("xyz", True, 6, R_NEAR), ("tilt", True, 6, R_NEAR), ("open", False, 4, R_NEAR),
            ("xyz", False, 12, R_FAR), ("xyz", False, 1, R_FAR), ("xyz", False, 3, R_FAR),
            # a lone bond: a row's errors have nothing to average with, and the recurrence is longest at l = 12
            ("dimers", False, 5, 1.3), ("dimers", False, 8, 1.3), ("dimers", False, 11, 1.3), ("dimers", False, 12, 1.3)]


@functools.lru_cache(maxsize=None)
def _dimer_ref(l):
    q, box6, mask = _dimers()
    return us.reference(q, box6, mask, l, 1.3, pairs=_dimer_pairs())


def _emulated(case, T, seed, defect=None):
    box, drift, l, r_max = case
    if box == "dimers":
        ref, q = _dimer_ref(l), _dimers()[0]
    else:
        ref, q = _ref(box, drift, l, r_max), _input(box, drift, r_max)
    return ref, us.emulate(q, l, T, np.random.default_rng(seed), ref["pairs"], defect=defect)


def test_emulation_gives_c():
    """STEIN_C is 4 x the largest ratio of the float32 emulation, family by family (the 4: the device's other order)."""
    worst = {"qlm": 0.0, "q": 0.0, "w": 0.0}
    for k, case in enumerate(EMULATED):
        ref, got = _emulated(case, np.float32, 100 + k)
        assert np.array_equal(got["nb"], ref["nb"])
        r = us.ratios(got, ref, np.float32, average=not (case[0] == "dimers" and case[2] % 2))  # (test_isolated_dimers says why)
        print(case, {key: round(v, 3) for key, v in r.items()})
        worst = {key: max(worst[key], r[key]) for key in worst}
    print("emulated:", worst, "STEIN_C:", us.STEIN_C)
    for key, v in worst.items():
        assert 4 * v <= us.STEIN_C[key] <= 4 * v * 1.1, (key, v)


def test_reference_error():
    """REF_C is 2 x the largest ratio, in units of 2^-53 S, of the float64 reference against the rule in long double."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    worst = {"qlm": 0.0, "q": 0.0, "w": 0.0}
    for k, case in enumerate(EMULATED[1:5]):
        ref, got = _emulated(case, np.longdouble, 200 + k)
        r = us.ratios(got, ref, np.float64)
        print(case, {key: round(v, 3) for key, v in r.items()})
        worst = {key: max(worst[key], r[key]) for key in worst}
    print("reference:", worst, "REF_C:", us.REF_C)
    for key, v in worst.items():
        assert 2 * v <= us.REF_C[key] <= 2 * v * 1.1, (key, v)


def test_emulation_in_float64_is_within_c():
    ref, got = _emulated(EMULATED[1], np.float64, 7)
    us.check(got, ref, np.float64)


@pytest.mark.parametrize("defect", us.DEFECTS)
def test_checker_refuses(defect):
    case = ("xyz", False, 3, R_FAR) if defect.startswith("r_i") else EMULATED[0]  # (the bond's direction shows at an odd l)
    ref, got = _emulated(case, np.float32, 3, defect)
    with pytest.raises(AssertionError):
        us.check(got, ref, np.float32)


def test_inputs_are_off_the_band():
    """No input has a pair within 2^-17 of r_max^2, and no particle is without neighbours: N_b is compared exactly and no
    particle is left out."""
    for r_max, span in ((R_NEAR, (3, 9)), (R_FAR, (6, 26))):
        lo, hi = N, 0
        for box in LJ_BOXES:
            I, _, d, _ = _pairs(box, False, r_max)  # (asserts the band)
            nb = np.bincount(I[(d * d).sum(axis=1) < r_max * r_max], minlength=N)
            print(box, r_max, "N_b", nb.min(), "..", nb.max())
            lo, hi = min(lo, nb.min()), max(hi, nb.max())
        assert (lo, hi) == span  # (the corners of the open box have the fewest)
    cols = _ref("xyz", False, 4)["cols"]
    q6 = _ref("xyz", False, 6)["cols"][:, 0]
    print("q4", cols[:, 0].min(), cols[:, 0].max(), "q6", q6.min(), q6.max())
    assert np.isfinite(_ref("xyz", False, 4)["S"]).all()


def test_classify_names_the_shells():
    v = np.array(list(st.CRYSTALS.values()))
    idx, dist = st.classify(v[:, 0], v[:, 1], v[:, 2], v[:, 3])
    assert np.array_equal(idx, np.arange(len(v))) and np.all(dist == 0)
    assert st.classify([np.nan], [0.5], [0.0], [0.0])[0][0] == -1


# ---------------------------------------------------------------------------------------------------------- GPU tests
def _built(q, box, dtype, rc, l, r_max, off=0, stride=4, skin=0.0, w=True, types=None, exclusions=None, full=True):
    """(handle, device positions) after one build, the setting made."""
    torch = _torch()
    nl = _handle(box, dtype, full, rc, off) if isinstance(box, str) else _box_handle(box, dtype, rc, off)
    if skin:
        nl.set_skin(skin)
    nl.Initialize(len(q))
    if types is not None:
        nl.set_type_cutoffs(*types)
    if exclusions is not None:
        nl.set_exclusions(exclusions, len(q))
    nl.set_steinhardt(l, r_max, w=w)
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


def _box_handle(box, dtype, rc, off=0):
    from md_neighbor_list_amd import NeighListGPU

    box6, mask = box
    nl = NeighListGPU(rc, *box6[:3], dtype=_tdt(dtype), full_list=True, minimum_image=tuple(bool(mask >> a & 1) for a in range(3)))
    if off:
        nl.set_offset_width(off)
    return nl


def device_result(nl, cols):
    """What the checker takes: the four columns with q_lm and N_b of the call that wrote them."""
    qlm, nb = nl.steinhardt_qlm()
    return {"cols": cols.cpu().numpy().astype(np.float64), "qlm": qlm.cpu().numpy().astype(np.complex128), "nb": nb.cpu().numpy()}


def _run(nl, qd, ref, dtype, average=True, wait=True, w=True, rows=None):
    cols = nl.steinhardt(qd, average=average, wait=wait)
    _torch().cuda.synchronize()
    assert cols.shape == (len(qd), 4) and cols.dtype == _tdt(dtype)
    r = us.check(device_result(nl, cols), ref, dtype, average, w, rows)
    print("reached", np.dtype(dtype).name, {k: round(v, 3) for k, v in r.items()})
    return cols


@gpu
@pytest.mark.parametrize("l", [4, 6])
@pytest.mark.parametrize("box,drift", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity(dtype, box, drift, l):
    nl, qd = _built(_input(box, drift), box, dtype, RC[R_NEAR], l, R_NEAR)
    _run(nl, qd, _ref(box, drift, l), dtype)


@gpu
@pytest.mark.parametrize("l", [1, 2, 3, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_of_other_degrees(dtype, l):
    """l = 1, 2, 3 and 12 on "xyz" at r_max = 2.0 (6 .. 26 neighbours), positions of stride 3."""
    nl, qd = _built(_input("xyz", False, R_FAR), "xyz", dtype, RC[R_FAR], l, R_FAR, stride=3)
    _run(nl, qd, _ref("xyz", False, l, R_FAR), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_reuse_within_the_skin(dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variant; no extra build."""
    torch = _torch()
    nl = _handle("xyz", dtype, True, 1.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    nl.set_steinhardt(6, R_NEAR)
    qd = torch.from_numpy(_input("xyz", False).astype(dtype)).cuda()
    nl.update(qd, sync=True)
    builds = nl.update_stats()[1]
    nl.steinhardt(qd)  # (the scratch)
    qd.copy_(torch.from_numpy(_moved().astype(dtype)))
    nl.update(qd)
    _run(nl, qd, _moved_ref(6), dtype, wait=False)
    assert nl.update_stats()[1] == builds


CRYSTAL_CASES = [("fcc", 4, 1.35, 1.5, "fcc"), ("hcp", 4, None, 2.0, "hcp"), ("bcc", 4, None, 1.55, "bcc"), ("bcc", 4, "second", 2.0, "bcc14"),
                 ("sc", 4, None, 2.0, "sc")]


@gpu
@pytest.mark.parametrize("name,cells,r_max,rc,shell", CRYSTAL_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_crystals(dtype, name, cells, r_max, rc, shell):
    """Perfect periodic lattices: every atom has the table's q4, q6, w4, w6 within the bound, and the averaged q_l is q_l."""
    q, box6, r1, r2 = us.crystal(name, cells)
    r_max = r2 if r_max == "second" else r1 if r_max is None else r_max
    pairs = lj_pairs(q, box6, 7, r_max)
    nbs = {"fcc": 12, "hcp": 12, "bcc": 8, "bcc14": 14, "sc": 6}[shell]
    for k, l in enumerate((4, 6)):
        ref = us.reference(q, box6, 7, l, r_max, pairs=pairs)
        assert np.all(ref["nb"] == nbs)
        want = np.array(st.CRYSTALS[shell])[[k, 2 + k, k, 2 + k]]
        assert np.abs(ref["cols"] - want).max() < 2e-6  # (the reference at these positions: the table, to float32 coordinates)
        nl, qd = _built(q, (box6, 7), dtype, rc, l, r_max)
        cols = _run(nl, qd, ref, dtype).cpu().numpy().astype(np.float64)
        u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
        bound = us.STEIN_C["q"] * u * ref["S"][:, [0, 2]].sum(axis=1)  # (the bounds of the two columns, and what the reference itself sees)
        assert np.all(np.abs(cols[:, 2] - cols[:, 0]) <= bound + np.abs(ref["cols"][:, 2] - ref["cols"][:, 0]))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolated_dimers(dtype):
    """A single bond has q_l = 1 and w_l = (l l l; 0 0 0) for every l, whatever its direction; the axes are among them.  The
    average runs at the even l: the partner sees the bond reversed, Y_lm(-u) = (-1)^l Y_lm(u), so at an odd l the averaged q_lm
    of a dimer is 0 and its w_l is 0 / 0."""
    q, box6, mask = _dimers()
    nl, qd = _built(q, (box6, mask), dtype, 1.5, 1, 1.3)
    for l in range(1, st.MAX_L + 1):
        nl.set_steinhardt(l, 1.3)
        ref = us.reference(q, box6, mask, l, 1.3, pairs=_dimer_pairs())
        used = [0, 1, 2, 3] if l % 2 == 0 else [0, 1]
        assert np.all(ref["nb"] == 1) and np.abs(ref["cols"][:, used[0::2]] - 1).max() < 1e-12
        assert np.abs(ref["cols"][:, used[1::2]] - st.wigner3j_table(l)[l, l]).max() < 1e-12
        cols = _run(nl, qd, ref, dtype, average=l % 2 == 0).cpu().numpy()
        assert np.isfinite(cols[:, used]).all()


@gpu
@pytest.mark.parametrize("off", [32, 64])
def test_long_rows(off):
    """About 113 neighbours a row: the walk takes two or more trips; both offset widths."""
    q, box6, mask, ref = _long_rows()
    assert ref["nb"].max() > 128 and ref["nb"].mean() > 100
    nl, qd = _built(q, (box6, mask), np.float32, 3.3, 6, 3.0, off=off)
    assert nl.build_info()["offset_bits"] == off
    _run(nl, qd, ref, np.float32)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_filtered_lists(dtype):
    """An exclusion table, and a type table with rc(0, nt - 1) = 0: the excluded partners and the partners of that pair of types
    are no neighbours."""
    box6, mask = LJ_BOXES["xyz"]
    q = _input("xyz", False)
    ex = _bonds()
    ref = us.reference(q, box6, mask, 6, R_NEAR, exclusions=ex, pairs=_pairs("xyz", False))
    assert (ref["nb"] < _ref("xyz", False, 6)["nb"]).sum() > N // 2
    nl, qd = _built(q, "xyz", dtype, RC[R_NEAR], 6, R_NEAR, exclusions=ex)
    _run(nl, qd, ref, dtype)
    types, rc_ab = lj_type_params(3, RC[R_NEAR])[:2]
    assert rc_ab[0, 2] == 0 and rc_ab[0, 0] == RC[R_NEAR]
    ref = us.reference(q, box6, mask, 6, R_NEAR, types=types, rc_ab=rc_ab, pairs=_pairs("xyz", False))
    assert (ref["nb"] < _ref("xyz", False, 6)["nb"]).sum() > N // 4
    nl, qd = _built(q, "xyz", dtype, RC[R_NEAR], 6, R_NEAR, types=(types, rc_ab))
    _run(nl, qd, ref, dtype)


@gpu
def test_no_neighbour_gives_nan():
    """A particle with partners within rc but none within r_max: NaN in its row and its q_lm, everybody else as the reference."""
    box6, mask = LJ_BOXES["xyz"]
    q0 = _input("xyz", False)
    c = N // 2 + 7 * 14 + 7
    I, J, d, _ = lj_pairs(q0, box6, mask, 1.7, rows=[c])
    q = np.delete(q0, J, axis=0)
    c -= int((J < c).sum())
    ref = us.reference(q, box6, mask, 6, R_NEAR)
    assert ref["nb"][c] == 0 and (ref["nb"] == 0).sum() == 1 and np.isnan(ref["cols"][c]).all()
    assert len(lj_pairs(q, box6, mask, RC[R_FAR], rows=[c])[0]) > 0
    nl, qd = _built(q, "xyz", np.float32, RC[R_FAR], 6, R_NEAR)
    cols = _run(nl, qd, ref, np.float32).cpu().numpy()
    qlm = nl.steinhardt_qlm()[0].cpu().numpy()
    assert np.isnan(cols[c]).all() and np.isnan(qlm[c].real).all() and np.isnan(qlm[c].imag).all()
    assert np.isfinite(np.delete(cols, c, axis=0)).all() and np.isfinite(np.delete(qlm, c, axis=0).view(np.float32)).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_the_same_bytes(dtype):
    torch = _torch()
    nl, qd = _built(_input("xyz", False, R_FAR), "xyz", dtype, RC[R_FAR], 6, R_FAR)
    a = nl.steinhardt(qd, average=True)
    qa, na = nl.steinhardt_qlm()
    b = nl.steinhardt(qd, average=True)
    qb, nb = nl.steinhardt_qlm()
    it = torch.int32 if dtype == np.float32 else torch.int64
    assert torch.equal(a.view(it), b.view(it)) and torch.equal(torch.view_as_real(qa).view(it), torch.view_as_real(qb).view(it))
    assert torch.equal(na, nb)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_columns_and_no_3j_table(dtype):
    """average = 0: columns 0 and 1 as with average = 1, columns 2 and 3 NaN (written, not left).  No 3j table: the w columns
    NaN, the q columns unchanged."""
    torch = _torch()
    it = torch.int32 if dtype == np.float32 else torch.int64
    nl, qd = _built(_input("xyz", False), "xyz", dtype, RC[R_NEAR], 4, R_NEAR)
    full = nl.steinhardt(qd, average=True)
    out = torch.full((N, 4), 5.0, dtype=_tdt(dtype), device="cuda")
    nl.steinhardt(qd, average=False, out=out)
    assert torch.equal(out[:, :2].contiguous().view(it), full[:, :2].contiguous().view(it)) and torch.isnan(out[:, 2:]).all()
    nl.set_steinhardt(4, R_NEAR, w=False)
    assert nl.steinhardt_info() == {"l": 4, "r_max": R_NEAR, "w": False}
    out.fill_(5.0)
    nl.steinhardt(qd, average=True, out=out)
    assert torch.equal(out[:, [0, 2]].contiguous().view(it), full[:, [0, 2]].contiguous().view(it)) and torch.isnan(out[:, [1, 3]]).all()
    _run(nl, qd, _ref("xyz", False, 4), dtype, w=False)


@gpu
def test_captured():
    """One graph holds the copy of the positions, the update and the call; replayed at two position sets.  A first call inside a
    capture is NL_ERR_STATE: the scratch does not exist yet."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()
    dtype = np.float32
    sets = [(_input("xyz", False), _ref("xyz", False, 6)), (_moved(), _moved_ref(6))]
    nl = _handle("xyz", dtype, True, 1.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    nl.set_steinhardt(6, R_NEAR)
    src = torch.from_numpy(sets[0][0].astype(dtype)).cuda()
    qd = src.clone()
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    nl.update(qd, sync=True)
    nl.update(qd)
    nl.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):
        with pytest.raises(NLError) as e:
            nl.steinhardt(qd, average=True, wait=False, out=out)
        assert e.value.code == NL_ERR_STATE
        qd.copy_(src)
    nl.steinhardt(qd, average=True, out=out)  # synchronous, outside a capture: allocates
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        nl.steinhardt(qd, average=True, wait=False, out=out)
    for q, ref in sets:
        src.copy_(torch.from_numpy(q.astype(dtype)))
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        us.check(device_result(nl, out), ref, dtype)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN in all four columns, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat the values are finite."""
    from md_neighbor_list_amd import NeighListGPU, inputs
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=True)
    nl.set_skin(0.4)
    nl.Initialize(len(q))
    nl.set_steinhardt(6, 2.0)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    nl.steinhardt(qd)  # (the scratch)
    nl.set_capacity(1000)
    nl.update(qd)
    cols = nl.steinhardt(qd, average=True, wait=False)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert torch.isnan(cols).all() and cols.shape == (len(q), 4)
    nl.update(qd, sync=True)  # grows the list
    cols = nl.steinhardt(qd, average=True, wait=False)
    torch.cuda.synchronize()
    assert torch.isfinite(cols).all()  # (at density 0.91 every particle has neighbours within 2.0)


@gpu
def test_half_slab_and_distributed_lists_are_refused():
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError
    from tests.test_slab_paths import slab_parts

    torch = _torch()
    box, dtype, rc = "xyz", np.float32, 3.4
    box6, mask = LJ_BOXES[box]
    q = _input(box, False)
    # a half list
    nl, qd = _built(q, box, dtype, rc, 6, R_NEAR, full=False)
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            nl.steinhardt(qd, wait=wait)
        assert e.value.code == NL_ERR_STATE
    # slab lists, local-index ones included
    part = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 2), (2, 4)), mask)[0]
    for local in (True, False):
        nl = _handle(box, dtype, True, rc)
        nl.set_local_ids(local)
        nl.Initialize(N)
        nl.set_steinhardt(6, R_NEAR)
        qs = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
        nl.MakeNeighListSlab(qs, None, len(part["own"]), part["z_lo"], part["z_hi"])
        out = torch.empty((len(qs), 4), dtype=torch.float32, device="cuda")
        for name in ("nl_steinhardt", "nl_steinhardt_enqueue"):
            assert getattr(nl._lib, name)(nl._h, qs.data_ptr(), 4, 1, out.data_ptr(), None) == NL_ERR_STATE
    # a distributed build of a world of one
    nl = _handle(box, dtype, True, rc)
    nl.Initialize(N)
    nl.set_steinhardt(6, R_NEAR)
    lib = nl._lib
    qg = q.astype(np.float32)
    qg[:, 3] = np.arange(N, dtype=np.int32).view(np.float32)  # NL_GID_IN_W
    qgd = torch.from_numpy(qg).cuda()
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    cb = _lib.SENDRECV_FN(lambda *a: 1)  # (never called: a world of one exchanges nothing)
    comm = C.c_void_p()
    assert lib.nl_comm_create_callbacks(C.byref(comm), 0, 1, cb, None, torch.cuda.current_device()) == 0
    try:
        assert lib.nl_make_list_distributed(nl._h, comm, qgd.data_ptr(), N, N, None, 1) == 0
        for name in ("nl_steinhardt", "nl_steinhardt_enqueue"):
            assert getattr(lib, name)(nl._h, qgd.data_ptr(), 4, 1, out.data_ptr(), None) == NL_ERR_STATE
    finally:
        lib.nl_comm_destroy(comm)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_on_a_callers_held_stream(dtype):
    """A non-blocking stream of the caller's, held back by a delay: the positions are written behind the delay, and the update
    and the call enqueued on that stream read what was written."""
    from tests.stream_util import device, held_stream, rolled

    torch = _torch()
    q = _input("xyz", False)
    nl = _handle("xyz", dtype, True, 1.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    nl.set_steinhardt(6, R_NEAR)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    qd = dec.clone()
    out = torch.empty((N, 4), dtype=_tdt(dtype), device="cuda")
    nl.update(qd, sync=True)  # (warm, on the decoy: nothing allocates while the stream is held)
    nl.steinhardt(qd, average=True, wait=False, out=out)
    nl.steinhardt(qd, average=True)
    torch.cuda.synchronize()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        nl.steinhardt(qd, average=True, wait=False, out=out)
        h.assert_held(f"steinhardt {np.dtype(dtype).name}")
    nl.synchronize()
    us.check(device_result(nl, out), _ref("xyz", False, 6), dtype)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    q = _input("open", False)
    nl = _handle("open", np.float32, True, 1.9)
    nl.set_skin(0.25)  # (1.9 - 0.25 is 1.65 in double as well)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    calls = [lib.nl_steinhardt, lib.nl_steinhardt_enqueue]
    # before a setting, before a build, before a call
    assert nl.steinhardt_info() is None
    p, c, n, l = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
    assert lib.nl_steinhardt_get_qlm(nl._h, C.byref(p), C.byref(c), C.byref(n), C.byref(l)) == NL_ERR_STATE
    nl.set_steinhardt(6, R_NEAR)
    for fn in calls:
        assert fn(nl._h, qd.data_ptr(), 4, 1, out.data_ptr(), None) == NL_ERR_STATE  # no list
    nl.update(qd, sync=True)
    nl.clear_steinhardt()
    for fn in calls:
        assert fn(nl._h, qd.data_ptr(), 4, 1, out.data_ptr(), None) == NL_ERR_STATE  # no setting
    nl.set_steinhardt(6, R_NEAR)
    assert nl.steinhardt_info() == {"l": 6, "r_max": R_NEAR, "w": True}
    # the calls' arguments
    for fn in calls:
        assert fn(nl._h, qd.data_ptr(), 4, 1, None, None) == NL_ERR_ARG
        assert fn(nl._h, None, 4, 1, out.data_ptr(), None) == NL_ERR_ARG
        assert fn(None, qd.data_ptr(), 4, 1, out.data_ptr(), None) == NL_ERR_ARG
        for stride in (0, 2, 5):
            assert fn(nl._h, qd.data_ptr(), stride, 1, out.data_ptr(), None) == NL_ERR_ARG
    # the setter's arguments: the old setting is kept
    w = st.wigner3j_table(6)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    bad = w.copy()
    bad[3, 4] = np.inf
    for args in ((-1, 1.0, wp), (13, 1.0, None), (6, 0.0, wp), (6, -1.0, wp), (6, np.inf, wp), (6, np.nan, wp),
                 (6, 1.0, bad.ctypes.data_as(C.POINTER(C.c_double)))):
        assert lib.nl_set_steinhardt(nl._h, *args) == NL_ERR_ARG, args[:2]
    assert lib.nl_set_steinhardt(None, 6, 1.0, wp) == NL_ERR_ARG
    assert nl.steinhardt_info() == {"l": 6, "r_max": R_NEAR, "w": True}
    # the setter keeps the list: an update after it builds nothing
    builds = nl.update_stats()[1]
    nl.set_steinhardt(4, R_NEAR)
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == builds
    assert torch.isfinite(nl.steinhardt(qd, average=True)).all()
    qlm, nb = nl.steinhardt_qlm()
    assert qlm.shape == (N, 5) and nb.shape == (N,) and nb.dtype == torch.int32
    # reach: rc = 1.9, skin = 0.25 -- 1.6 and 1.65 are within rc - skin, 1.7 and 1.9 only within rc, 2.0 within neither
    assert 1.9 - 0.25 == 1.65
    for r_max, sync_ok, enq_ok in ((1.6, True, True), (1.65, True, True), (1.7, True, False), (1.9, True, False), (2.0, False, False)):
        nl.set_steinhardt(4, r_max)
        for wait, ok in ((True, sync_ok), (False, enq_ok)):
            if ok:
                nl.steinhardt(qd, wait=wait)
            else:
                with pytest.raises(NLError) as e:
                    nl.steinhardt(qd, wait=wait)
                assert e.value.code == NL_ERR_ARG, (r_max, wait)
    # with a type table: a pair of types with rc_ab = 0 asks for nothing, another short of r_max is refused
    types = (np.arange(N) % 3).astype(np.int32)
    nl.set_type_cutoffs(types, [[1.9, 1.9, 0.0], [1.9, 1.65, 1.9], [0.0, 1.9, 1.9]])
    nl.MakeNeighList(qd, N)
    nl.set_steinhardt(4, 1.6)
    nl.steinhardt(qd)
    with pytest.raises(NLError) as e:
        nl.steinhardt(qd, wait=False)  # 1.6 > 1.65 - 0.25
    assert e.value.code == NL_ERR_ARG
    # clearing, both ways
    nl.clear_steinhardt()
    assert nl.steinhardt_info() is None
    nl.set_steinhardt(4, 1.6)
    assert lib.nl_set_steinhardt(nl._h, 0, 1.6, wp) == 0 and nl.steinhardt_info() is None
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            nl.steinhardt(qd, wait=wait)
        assert e.value.code == NL_ERR_STATE
    # n == 0: the call succeeds and writes nothing
    empty = _handle("open", np.float32, True, 1.9)
    empty.Initialize(16)
    empty.set_steinhardt(4, 1.6)
    empty.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    out.fill_(7.0)
    assert lib.nl_steinhardt(empty._h, qd.data_ptr(), 4, 1, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # a larger l after a call, and another n_max: the scratch is made anew by the next call
    nl2, qd2 = _built(_input("xyz", False), "xyz", np.float32, RC[R_NEAR], 4, R_NEAR)
    nl2.steinhardt(qd2)
    nl2.set_steinhardt(12, R_NEAR)
    _run(nl2, qd2, _ref("xyz", False, 12), np.float32)
    nl2.Initialize(N + 100)
    assert lib.nl_steinhardt_get_qlm(nl2._h, C.byref(p), C.byref(c), C.byref(n), C.byref(l)) == NL_ERR_STATE
    nl2.MakeNeighList(qd2, N)
    _run(nl2, qd2, _ref("xyz", False, 12), np.float32)

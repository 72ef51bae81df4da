"""Common neighbour analysis from the list (nl_cna, nl_cna_enqueue).

The contract.  The type and all eight counts words of every particle equal the O(N^2) float64 evaluation of the header's rule
(tests.util_cna) wherever none of the particle's decisions lies within 2^-17 (fp32; 2^-46 fp64; relative, r^2) of its threshold
(`sure`); the summary equals the histogram of the device's own types at all particles.  The condition under which equality is
demanded -- at least 98 % of the particles of every input used on the GPU are sure -- is asserted by the CPU test
test_inputs_are_sure.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from md_neighbor_list_amd import cna
from tests import util_cna as uc
from tests.consumer_util import DTYPES, _tdt, _torch

gpu = pytest.mark.gpu
MODES = (False, True)  # adaptive
A_FCC, D_HCP, A_BCC = 1.6, 1.1, 1.3  # fcc and bcc: the cubic lattice constant; hcp: the neighbour distance


def _f32(p):
    return np.asarray(p, dtype=np.float64).astype(np.float32).astype(np.float64)


def _wrap(p, box6):
    """Into the (triclinic) cell, z first."""
    Lx, Ly, Lz, xy, xz, yz = box6
    p = p.copy()
    k = np.floor(p[:, 2] / Lz)
    p -= k[:, None] * np.array([xz, yz, Lz])
    k = np.floor(p[:, 1] / Ly)
    p -= k[:, None] * np.array([xy, Ly, 0.0])
    k = np.floor(p[:, 0] / Lx)
    p -= k[:, None] * np.array([Lx, 0.0, 0.0])
    return p


def _q4(p):
    q = np.zeros((len(p), 4))
    q[:, :3] = _f32(p)
    q.setflags(write=False)
    return q


# ---------------------------------------------------------------------------------------------------------- the inputs
# name: (lattice kind, cells, lattice constant, nearest-neighbour distance, rc of the list in lattice constants, type)
CRYSTALS = {
    "fcc": ("fcc", 4, A_FCC, A_FCC * np.sqrt(0.5), 0.95, uc.FCC),        # 256 atoms, box 4 a, mesh 4
    "hcp": ("hcp", (6, 4, 4), D_HCP, D_HCP, 1.5, uc.HCP),               # 384 atoms, box (6, 6.93, 6.53) d, mesh 4
    "bcc": ("bcc", 5, A_BCC, A_BCC * np.sqrt(0.75), 1.3, uc.BCC),        # 250 atoms, box 5 a, mesh 3
    "fcc_wide": ("fcc", 4, A_FCC, A_FCC * np.sqrt(0.5), 1.3, uc.FCC),   # the list reaches the third shell: 42 candidates, mesh 3
}


@functools.lru_cache(maxsize=None)
def _crystal(name, jitter=0.03, offset=0.25, seed=5, tilt=0.0):
    """(q (n, 4) float64 holding float32 values, box6, mask 7, rc): the lattice of CRYSTALS[name] moved by `offset` cells,
    every atom displaced by a Gaussian of `jitter` nearest-neighbour distances per axis, wrapped, in shuffled order.  tilt: xy in
    lattice constants -- the same positions in the sheared cell, a lattice-compatible tilt."""
    kind, cells, a, nn, rc, _ = CRYSTALS[name]
    p, box = cna.lattice(kind, cells, a)
    rng = np.random.default_rng(seed)
    p = p + offset * a + rng.normal(0.0, jitter * nn, size=p.shape) if jitter else p + offset * a
    box6 = (float(np.float32(box[0])), float(np.float32(box[1])), float(np.float32(box[2])), float(np.float32(tilt * a)), 0.0, 0.0)
    p = _wrap(p, box6)[rng.permutation(len(p))]
    return _q4(p), box6, 7, rc * a


def _r_max(name, adaptive):
    """Fixed: the conventional cut-off; adaptive: everything the list holds."""
    kind, _, a, _, rc, _ = CRYSTALS[name]
    return rc * a if adaptive else cna.default_r_max(kind, a)


@functools.lru_cache(maxsize=None)
def _crystal_ref(name, adaptive, dtype, **kw):
    q, box6, mask, _ = _crystal(name, **kw)
    return uc.reference(q, box6, mask, _r_max(name, adaptive), adaptive, dtype)


FAULT = "ABCABCBCABC"  # one intrinsic stacking fault: the layers 5 (C between B and B) and 6 (B between C and C) are hcp


@functools.lru_cache(maxsize=None)
def _fault():
    """(q, box6, mask, rc, layer): 11 close-packed layers of 48 atoms, fcc with one layer taken out."""
    p, box, layer = cna.stacked(FAULT, 6, 4, D_HCP)
    box6 = tuple(float(np.float32(b)) for b in box) + (0.0, 0.0, 0.0)
    return _q4(_wrap(p + 0.2, box6)), box6, 7, 1.5 * D_HCP, layer


@functools.lru_cache(maxsize=None)
def _ico():
    """(q, box6, mask 0, rc): the 13-atom icosahedron of radius 1 in the middle of an open box of edge 12, and a sparse grid of
    filler (spacing 3, nobody within 1.5 of anybody) that gives the mesh its extent."""
    g = np.stack(np.meshgrid(*(np.arange(4),) * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 3.0 + 1.5
    g = g[np.linalg.norm(g - 6.0, axis=1) > 4.0]
    p = np.concatenate([cna.icosahedron(1.0) + 6.0, g])
    return _q4(p), (12.0, 12.0, 12.0, 0.0, 0.0, 0.0), 0, 1.5


@functools.lru_cache(maxsize=None)
def _liquid():
    """(q, box6, mask, rc): 500 particles at density 0.85 with no pair closer than 0.8, placed one after the other at random;
    within R_LIQ = 1.69 a particle has about 10 to 23 neighbours."""
    n, L, dmin = 500, (500 / 0.85) ** (1.0 / 3.0), 0.8
    rng = np.random.default_rng(12)
    p = np.zeros((0, 3))
    while len(p) < n:
        c = rng.uniform(0.0, L, size=3)
        d = p - c
        d -= L * np.rint(d / L)
        if not len(p) or (d * d).sum(axis=1).min() > dmin * dmin:
            p = np.concatenate([p, c[None]])
    Lf = float(np.float32(L))
    return _q4(np.minimum(p, 0.999 * Lf)), (Lf, Lf, Lf, 0.0, 0.0, 0.0), 7, 1.7


R_LIQ = 1.69
R_STAR = 1.0


@functools.lru_cache(maxsize=None)
def _stars():
    """(q, box6, mask, rc, centres): four stars, a centre with 63, 64, 66 and 70 particles in the shell 0.7 .. 0.95 around it (all
    within R_STAR = 1.0 of the centre, about a third of them within it of each other), 3.5 apart in a periodic box of edge 8
    with 150 random filler particles that stay 1.2 clear of the centres.  centres: {index: number on its sphere}."""
    rng = np.random.default_rng(8)
    L = 8.0
    cs = np.array([[2.0, 2.0, 2.0], [5.5, 2.0, 2.0], [2.0, 5.5, 2.0], [2.0, 2.0, 5.5]]) + 0.1
    pts, centres = [], {}
    for c, m in zip(cs, (63, 64, 66, 70)):
        u = rng.normal(size=(m, 3))
        centres[sum(len(x) for x in pts)] = m
        pts += [c[None], c + (rng.uniform(0.7, 0.95, size=(m, 1)) * u) / np.linalg.norm(u, axis=1)[:, None]]
    fill = np.zeros((0, 3))
    while len(fill) < 150:
        c = rng.uniform(0.0, L, size=3)
        d = cs - c
        d -= L * np.rint(d / L)
        if (d * d).sum(axis=1).min() > 2.1 ** 2:
            fill = np.concatenate([fill, c[None]])
    p = np.concatenate(pts + [fill])
    order = rng.permutation(len(p))
    inv = np.argsort(order)
    return _q4(np.minimum(p[order], 0.999 * L)), (L, L, L, 0.0, 0.0, 0.0), 7, 1.2, {int(inv[i]): m for i, m in centres.items()}


@functools.lru_cache(maxsize=None)
def _ref(which, adaptive, dtype):
    q, box6, mask, rc = {"fault": _fault, "ico": _ico, "liquid": _liquid, "stars": _stars}[which]()[:4]
    r = {"fault": cna.default_r_max("hcp", D_HCP), "ico": 1.3, "liquid": R_LIQ, "stars": R_STAR}[which]
    if adaptive and which == "fault":
        r = rc
    return uc.reference(q, box6, mask, r, adaptive, dtype), r


# ---- the exclusion case: the wide fcc list, one neighbour of one FCC centre excluded
@functools.lru_cache(maxsize=None)
def _excluded_pair():
    """(centre, neighbour): a centre that is FCC and sure in both modes and types, and its nearest neighbour."""
    q, box6, mask, _ = _crystal("fcc_wide")
    ok = np.ones(len(q), dtype=bool)
    for adaptive in MODES:
        for dtype in DTYPES:
            ref = _crystal_ref("fcc_wide", adaptive, dtype)
            ok &= ref["sure"] & (ref["type"] == uc.FCC)
    c = int(np.flatnonzero(ok)[0])
    d = uc.separations(q[:, :3], box6, mask)[c]
    r2 = (d * d).sum(axis=1)
    r2[c] = np.inf
    return c, int(np.argmin(r2))


@functools.lru_cache(maxsize=None)
def _excluded_ref(adaptive, dtype):
    q, box6, mask, _ = _crystal("fcc_wide")
    return uc.reference(q, box6, mask, _r_max("fcc_wide", adaptive), adaptive, dtype, exclusions=np.array([_excluded_pair()]))


# ---------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("name", ["fcc", "hcp", "bcc"])
def test_reference_on_ideal_lattices(name, adaptive):
    for dtype in DTYPES:
        ref = _crystal_ref(name, adaptive, dtype, jitter=0.0)
        assert (ref["type"] == CRYSTALS[name][5]).all(), (name, adaptive)
        # (adaptive bcc: the six second neighbours are equally far, so who of them is in the 12-set is open -- and does not matter)
        assert ref["sure"].all() or (name == "bcc" and adaptive)
        assert ref["summary"][CRYSTALS[name][5]] == len(ref["type"]) and ref["summary"].sum() == len(ref["type"])
        nb, size = {"fcc": (12, 12), "hcp": (12 if not adaptive else 18, 12), "bcc": (14, 14)}[name]
        assert (ref["counts"][:, 0] == nb).all() and (ref["counts"][:, 1] == size).all() and not ref["counts"][:, 7].any()
        sig = {"fcc": [12, 0, 0, 0, 0], "hcp": [6, 6, 0, 0, 0], "bcc": [0, 0, 6, 0, 8]}[name]
        assert (ref["counts"][:, 2:7] == sig).all()


@pytest.mark.parametrize("adaptive", MODES)
def test_reference_on_the_icosahedron(adaptive):
    ref, _ = _ref("ico", adaptive, np.float64)
    assert ref["type"][0] == uc.ICO and ref["counts"][0].tolist() == [12, 12, 0, 0, 0, 12, 0, 0]
    assert (ref["type"][1:] == uc.OTHER).all() and (ref["counts"][1:13, 0] == 6).all() and (ref["counts"][13:, 0] == 0).all()


@pytest.mark.parametrize("adaptive", MODES)
def test_reference_on_the_stacking_fault(adaptive):
    """Exactly the two (111) layers next to the fault are hcp, the rest fcc."""
    layer = _fault()[4]
    ref, _ = _ref("fault", adaptive, np.float32)
    assert (ref["type"][np.isin(layer, (5, 6))] == uc.HCP).all() and (ref["type"][~np.isin(layer, (5, 6))] == uc.FCC).all()
    assert ref["summary"].tolist() == [0, 9 * 48, 2 * 48, 0, 0, 0] and ref["sure"].all()


def test_reference_on_the_stars():
    q, box6, mask, rc, centres = _stars()
    for adaptive in MODES:
        ref, _ = _ref("stars", adaptive, np.float32)
        for i, m in centres.items():
            assert ref["counts"][i, 0] == m and ref["counts"][i, 7] == (1 if m > 64 else 0)
            assert ref["counts"][i, 1] == (0 if m > 64 else 12 if adaptive else m) or (adaptive and ref["counts"][i, 1] == 14)
        assert ref["summary"][5] == 2 and ref["counts"][:, 0].max() == 70
        assert ref["type"][[i for i, m in centres.items() if m > 64]].tolist() == [uc.OTHER] * 2


def test_helpers():
    assert cna.NAMES[uc.FCC] == "fcc" and cna.NAMES[uc.HCP] == "hcp" and cna.NAMES[uc.BCC] == "bcc" and cna.NAMES[uc.ICO] == "ico"
    f = cna.fractions(np.array([1, 1, 2, 0, -1, 3, 3, 3], dtype=np.int32))
    assert f == {"other": 0.125, "fcc": 0.25, "hcp": 0.125, "bcc": 0.375, "ico": 0.0}
    assert abs(cna.default_r_max("fcc", 2.0) - (np.sqrt(2.0) + 2.0) / 2) < 1e-12 and abs(cna.default_r_max("bcc", 1.0) - uc.K) < 1e-12
    assert abs(cna.default_r_max("hcp", 1.0) - uc.K) < 1e-12
    with pytest.raises(ValueError):
        cna.default_r_max("sc", 1.0)
    with pytest.raises(ValueError):
        cna.stacked("ABA", 2, 2)
    v = cna.icosahedron(2.0)
    assert v.shape == (13, 3) and np.allclose(np.linalg.norm(v[1:], axis=1), 2.0) and not v[0].any()
    p, box, layer = cna.stacked("AB", 3, 2, 1.0)
    assert len(p) == 24 and np.allclose(box, [3.0, 2 * np.sqrt(3.0), 2 * np.sqrt(2.0 / 3.0)]) and layer.tolist() == [0] * 12 + [1] * 12


HOT = 0.07  # a jitter at which about half of the fcc atoms keep their type: every count word takes many values
GPU_INPUTS = ([("crystal", name, {}) for name in CRYSTALS]
              + [("crystal", "fcc", {"offset": 0.0}), ("crystal", "fcc", {"tilt": 1.0}), ("crystal", "fcc", {"jitter": HOT})]
              + [(w, None, {}) for w in ("fault", "ico", "liquid", "stars")])


def test_inputs_are_sure():
    """At every input used on the GPU at least 98 % of the particles are sure, in both modes and types; and the inputs are what
    their tests take them for."""
    for what, name, kw in GPU_INPUTS:
        for adaptive in MODES:
            for dtype in DTYPES:
                ref = _crystal_ref(name, adaptive, dtype, **kw) if what == "crystal" else _ref(what, adaptive, dtype)[0]
                frac = ref["sure"].mean()
                print(what, name, kw, "adaptive" if adaptive else "fixed", np.dtype(dtype).name, "sure", round(float(frac), 4),
                      "types", ref["summary"].tolist())
                assert frac >= 0.98, (what, name, kw, adaptive, dtype)
    for adaptive in MODES:
        for dtype in DTYPES:
            assert _excluded_ref(adaptive, dtype)["sure"].mean() >= 0.98
        for name in ("fcc", "hcp", "bcc"):
            ref = _crystal_ref(name, adaptive, np.float32)
            assert (ref["type"] == CRYSTALS[name][5]).mean() >= 0.9, (name, adaptive)
        assert (_crystal_ref("fcc_wide", True, np.float32)["type"] == uc.FCC).mean() >= 0.9
        nb = _ref("liquid", adaptive, np.float32)[0]["counts"][:, 0]
        assert nb.min() < 12 and nb.max() > 20 and 12 < nb.mean() < 20  # N_b straddles 12 .. 20
    # the sheared cell holds the same crystal: the same types as the orthogonal one
    for adaptive in MODES:
        a, b = _crystal_ref("fcc", adaptive, np.float32), _crystal_ref("fcc", adaptive, np.float32, tilt=1.0)
        both = a["sure"] & b["sure"]
        # (types, not counts: across the sheared face an atom meets the jitter of other atoms, so N_b may differ)
        assert np.array_equal(a["type"][both], b["type"][both])
    # the crystal without an offset has atoms on both sides of every face
    q, box6, _, _ = _crystal("fcc", offset=0.0)
    for ax in range(3):
        assert (q[:, ax] < 0.1).any() and (q[:, ax] > box6[ax] - 0.1).any()


# ---------------------------------------------------------------------------------------------------------- GPU tests
def _nl(box6, mask, dtype, rc, full=True, off=0):
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box6[:3], dtype=_tdt(dtype), full_list=full,
                      minimum_image=tuple(bool(mask >> a & 1) for a in range(3)) if mask else False, tilt=box6[3:])
    if off:
        nl.set_offset_width(off)
    return nl


def _built(q, box6, mask, dtype, rc, full=True, off=0, stride=4, exclusions=None):
    torch = _torch()
    nl = _nl(box6, mask, dtype, rc, full, off)
    nl.Initialize(len(q))
    if exclusions is not None:
        nl.set_exclusions(exclusions, len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    if off:
        assert nl.build_info()["offset_bits"] == off
    return nl, qd


def _host(t):
    return None if t is None else t.cpu().numpy()


def _cna(nl, qd, r_max, adaptive, **kw):
    out = nl.cna(qd, r_max, adaptive=adaptive, counts=True, summary=True, **kw)
    _torch().cuda.synchronize()
    return tuple(_host(t) for t in out)


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CRYSTALS))
def test_jittered_crystals(name, dtype, adaptive):
    q, box6, mask, rc = _crystal(name)
    nl, qd = _built(q, box6, mask, dtype, rc, off=64 if name == "hcp" else 32)
    ref = _crystal_ref(name, adaptive, dtype)
    got = _cna(nl, qd, _r_max(name, adaptive), adaptive)
    uc.check(*got, ref, (name, adaptive))
    print(name, "adaptive" if adaptive else "fixed", np.dtype(dtype).name, cna.fractions(got[0]))
    assert (got[0] == CRYSTALS[name][5]).mean() >= 0.9  # (the test cannot pass on all-OTHER)
    if name == "fcc_wide" and adaptive:
        assert (got[1][:, 0] > 30).all() and (got[1][:, 1] == 12).all()  # the 12 nearest of about 42 candidates


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hot_crystal(dtype, adaptive):
    """About half of the atoms keep their type, the others show every kind of broken signature."""
    q, box6, mask, rc = _hot()
    nl, qd = _built(q, box6, mask, dtype, rc, stride=3)
    ref = _crystal_ref("fcc", adaptive, dtype, jitter=HOT)
    got = _cna(nl, qd, _r_max("fcc", adaptive), adaptive)
    uc.check(*got, ref, "hot")
    assert 0.2 < (got[0] == uc.FCC).mean() < 0.8 and len(np.unique(got[1][:, 2])) > 4


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_stacking_fault_and_icosahedron(dtype, adaptive):
    q, box6, mask, rc, layer = _fault()
    ref, r = _ref("fault", adaptive, dtype)
    nl, qd = _built(q, box6, mask, dtype, rc)
    got = _cna(nl, qd, r, adaptive)
    uc.check(*got, ref, "fault")
    assert (got[0][np.isin(layer, (5, 6))] == uc.HCP).all() and got[2].tolist() == [0, 9 * 48, 2 * 48, 0, 0, 0]
    q, box6, mask, rc = _ico()
    ref, r = _ref("ico", adaptive, dtype)
    nl, qd = _built(q, box6, mask, dtype, rc, stride=3)
    got = _cna(nl, qd, r, adaptive)
    uc.check(*got, ref, "ico")
    assert got[0][0] == uc.ICO and got[2].tolist() == [len(q) - 1, 0, 0, 0, 1, 0]


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_liquid(dtype, adaptive):
    q, box6, mask, rc = _liquid()
    ref, r = _ref("liquid", adaptive, dtype)
    nl, qd = _built(q, box6, mask, dtype, rc)
    got = _cna(nl, qd, r, adaptive)
    uc.check(*got, ref, "liquid")
    print("liquid", "adaptive" if adaptive else "fixed", np.dtype(dtype).name, "OTHER fraction", cna.fractions(got[0])["other"],
          "sure", float(ref["sure"].mean()))


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow(dtype, adaptive):
    """Centres with 66 and 70 candidates: OTHER, flagged, counted in word 5, N_b exact; the centres with 63 and 64 are analysed."""
    q, box6, mask, rc, centres = _stars()
    ref, r = _ref("stars", adaptive, dtype)
    nl, qd = _built(q, box6, mask, dtype, rc)
    typ, cnt, sm = _cna(nl, qd, r, adaptive)
    uc.check(typ, cnt, sm, ref, "stars")
    for i, m in centres.items():
        assert cnt[i, 0] == m
        if m > 64:
            assert typ[i] == uc.OTHER and cnt[i].tolist() == [m, 0, 0, 0, 0, 0, 0, 1]
        else:
            assert cnt[i, 7] == 0 and cnt[i, 1] == ref["counts"][i, 1] > 0
    assert sm[5] == 2


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_triclinic_box(dtype, adaptive):
    """The fcc crystal in a cell sheared by one lattice constant: the oracle's answer in that cell, and the orthogonal one's."""
    q, box6, mask, rc = _crystal("fcc", tilt=1.0)
    assert abs(box6[3] - A_FCC) < 1e-6
    nl, qd = _built(q, box6, mask, dtype, rc)
    got = _cna(nl, qd, _r_max("fcc", adaptive), adaptive)
    uc.check(*got, _crystal_ref("fcc", adaptive, dtype, tilt=1.0), "tilt")
    orth = _crystal_ref("fcc", adaptive, dtype)
    assert np.array_equal(got[0][orth["sure"]], orth["type"][orth["sure"]])
    assert (got[0] == uc.FCC).mean() >= 0.9


@gpu
@pytest.mark.parametrize("adaptive", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairs_across_every_face(dtype, adaptive):
    q, box6, mask, rc = _crystal("fcc", offset=0.0)
    nl, qd = _built(q, box6, mask, dtype, rc)
    got = _cna(nl, qd, _r_max("fcc", adaptive), adaptive)
    uc.check(*got, _crystal_ref("fcc", adaptive, dtype, offset=0.0), "faces")
    assert (got[0] == uc.FCC).mean() >= 0.9


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_exclusion_table(dtype):
    """One neighbour of an FCC centre excluded: fixed, the centre has 11 candidates and is OTHER; adaptive, it is analysed on
    its 12 nearest other candidates."""
    q, box6, mask, rc = _crystal("fcc_wide")
    c, nb = _excluded_pair()
    nl, qd = _built(q, box6, mask, dtype, rc, exclusions=np.array([[c, nb]], dtype=np.int32))
    for adaptive in MODES:
        ref, whole = _excluded_ref(adaptive, dtype), _crystal_ref("fcc_wide", adaptive, dtype)
        typ, cnt, sm = _cna(nl, qd, _r_max("fcc_wide", adaptive), adaptive)
        uc.check(typ, cnt, sm, ref, ("excluded", adaptive))
        assert whole["type"][c] == uc.FCC and cnt[c, 0] == whole["counts"][c, 0] - 1 and cnt[nb, 0] == whole["counts"][nb, 0] - 1
        if adaptive:
            assert cnt[c, 1] in (12, 14) and cnt[c, 0] > 14 and ref["sure"][c]
        else:
            assert typ[c] == uc.OTHER and cnt[c, 0] == 11 and cnt[c, 1] == 11


# ---- the entry points' contract
SKIN = 0.1


def _skin_handle(dtype):
    """The hot fcc crystal's list with a skin: rc = 0.95 a = 1.52, reach 1.42 >= the fixed cut-off 1.366."""
    q, box6, mask, rc = _hot()
    nl = _nl(box6, mask, dtype, rc)
    nl.set_skin(SKIN)
    nl.Initialize(len(q))
    return nl


def _hot():
    return _crystal("fcc", jitter=HOT)


R_SKIN = {False: cna.default_r_max("fcc", A_FCC), True: 0.95 * A_FCC - SKIN}


@functools.lru_cache(maxsize=None)
def _moved():
    """The hot fcc crystal with every atom moved by up to 0.028 per axis: by less than skin / 2 = 0.05."""
    q, box6, mask, rc = _hot()
    m = q.copy()
    m[:, :3] = _f32(q[:, :3] + np.random.default_rng(21).uniform(-0.028, 0.028, size=(len(q), 3)))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _skin_ref(moved, adaptive, dtype):
    _, box6, mask, _ = _hot()
    return uc.reference(_moved() if moved else _hot()[0], box6, mask, R_SKIN[adaptive], adaptive, dtype)


def test_skin_inputs_are_sure():
    for moved in (False, True):
        for adaptive in MODES:
            for dtype in DTYPES:
                assert _skin_ref(moved, adaptive, dtype)["sure"].mean() >= 0.98
    # the moved positions give another answer: a replay that read the old ones would be seen
    assert not np.array_equal(_skin_ref(False, False, np.float32)["counts"], _skin_ref(True, False, np.float32)["counts"])
    assert not np.array_equal(_skin_ref(False, True, np.float32)["counts"], _skin_ref(True, True, np.float32)["counts"])


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_reuse_within_the_skin(dtype):
    """The enqueue variant behind nl_update_list, on a list kept within the skin, at moved positions; no extra build."""
    torch = _torch()
    nl = _skin_handle(dtype)
    qd = torch.from_numpy(_hot()[0].astype(dtype)).cuda()
    nl.update(qd, sync=True)
    builds = nl.update_stats()[1]
    qd.copy_(torch.from_numpy(_moved().astype(dtype)))
    nl.update(qd)
    outs = [nl.cna(qd, R_SKIN[adaptive], adaptive=adaptive, counts=True, wait=False) for adaptive in MODES]
    torch.cuda.synchronize()
    assert nl.update_stats()[1] == builds
    for adaptive, out in zip(MODES, outs):
        uc.check(*(_host(t) for t in out), _skin_ref(True, adaptive, dtype), ("skin", adaptive))


@gpu
def test_captured():
    """One graph holds the copy of the positions, the update and both analyses -- the first calls of the handle: nothing is
    allocated; replayed at two position sets."""
    torch = _torch()
    dtype = np.float32
    nl = _skin_handle(dtype)
    n = len(_hot()[0])
    src = torch.from_numpy(_hot()[0].astype(dtype)).cuda()
    qd = src.clone()
    nl.update(qd, sync=True)
    nl.update(qd)
    nl.synchronize()
    counts = [torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in MODES]
    summary = [torch.empty(6, dtype=torch.int64, device="cuda") for _ in MODES]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        types = [nl.cna(qd, R_SKIN[a], adaptive=a, counts=counts[k], summary=summary[k], wait=False)[0] for k, a in enumerate(MODES)]
    for moved in (False, True):
        src.copy_(torch.from_numpy((_moved() if moved else _hot()[0]).astype(dtype)))
        for t in types + counts + summary:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k, a in enumerate(MODES):
            uc.check(_host(types[k]), _host(counts[k]), _host(summary[k]), _skin_ref(moved, a, dtype), ("captured", moved, a))


@gpu
def test_failed_list():
    """Enqueued behind an asynchronous build that overflowed its capacity: -1 in every type, counts word and summary word;
    NL_ERR_CAPACITY at synchronize; after the synchronous repeat the answers are there."""
    from md_neighbor_list_amd import NeighListGPU, inputs
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = NeighListGPU(1.6, *box, dtype=torch.float32, full_list=True)
    nl.set_skin(0.1)
    nl.Initialize(len(q))
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    nl.set_capacity(1000)
    nl.update(qd)
    outs = [nl.cna(qd, 1.45, adaptive=a, counts=True, wait=False) for a in MODES]
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    for typ, cnt, sm in outs:
        assert (typ == -1).all() and (cnt == -1).all() and sm.tolist() == [-1] * 6
    nl.update(qd, sync=True)  # grows the list
    typ, cnt, sm = nl.cna(qd, 1.45, counts=True, wait=False)
    torch.cuda.synchronize()
    assert sm[:5].sum() == len(q) and np.array_equal(_host(sm[:5]), np.bincount(_host(typ), minlength=5)) and cnt[:, 0].sum() > 10 * len(q)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_bytes(dtype):
    """Two calls on one list write the same bytes, and so do two builds of one input (the outputs are integers of a rule that
    does not depend on the order of a row)."""
    torch = _torch()
    q, box6, mask, rc = _liquid()
    nl, qd = _built(q, box6, mask, dtype, rc)
    for adaptive in MODES:
        a = nl.cna(qd, R_LIQ, adaptive=adaptive, counts=True)
        b = nl.cna(qd, R_LIQ, adaptive=adaptive, counts=True)
        nl.MakeNeighList(qd, len(q))
        c = nl.cna(qd, R_LIQ, adaptive=adaptive, counts=True)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


@gpu
def test_refused_lists():
    """A half list, slab lists (local-index ones included) and a distributed build: NL_ERR_STATE from both entry points."""
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError
    from tests.consumer_util import N, _handle, _lj_input
    from tests.test_slab_paths import slab_parts
    from tests.util import LJ_BOXES

    torch = _torch()
    box, dtype, rc = "xyz", np.float32, 3.4
    box6, mask = LJ_BOXES[box]
    q = _lj_input(box, False)

    def all_refuse(nl, qp, n):
        typ = torch.empty(n, dtype=torch.int32, device="cuda")
        for name in ("nl_cna", "nl_cna_enqueue"):
            for mode in (0, 1):
                assert getattr(nl._lib, name)(nl._h, qp.data_ptr(), 4, mode, 1.5, typ.data_ptr(), None, None, None) == NL_ERR_STATE

    # a half list
    nlh = _handle(box, dtype, False, rc)
    nlh.Initialize(N)
    qh = torch.from_numpy(q.astype(dtype)).cuda()
    nlh.MakeNeighList(qh, N)
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            nlh.cna(qh, 1.5, wait=wait)
        assert e.value.code == NL_ERR_STATE
    all_refuse(nlh, qh, N)
    # slab lists
    part = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 2), (2, 4)), mask)[0]
    for local in (True, False):
        nls = _handle(box, dtype, True, rc)
        nls.set_local_ids(local)
        nls.Initialize(N)
        qs = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
        nls.MakeNeighListSlab(qs, None, len(part["own"]), part["z_lo"], part["z_hi"])
        all_refuse(nls, qs, len(qs))
    # a distributed build of a world of one
    nld = _handle(box, dtype, True, rc)
    nld.Initialize(N)
    qg = q.astype(np.float32)
    qg[:, 3] = np.arange(N, dtype=np.int32).view(np.float32)  # NL_GID_IN_W
    qgd = torch.from_numpy(qg).cuda()
    cb = _lib.SENDRECV_FN(lambda *a: 1)  # (never called: a world of one exchanges nothing)
    comm = C.c_void_p()
    assert nld._lib.nl_comm_create_callbacks(C.byref(comm), 0, 1, cb, None, torch.cuda.current_device()) == 0
    try:
        assert nld._lib.nl_make_list_distributed(nld._h, comm, qgd.data_ptr(), N, N, None, 1) == 0
        all_refuse(nld, qgd, N)
    finally:
        nld._lib.nl_comm_destroy(comm)


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    q, box6, mask, rc = _crystal("bcc")  # rc = 1.69
    n = len(q)
    nl = _nl(box6, mask, np.float32, rc)
    nl.set_skin(0.25)
    nl.Initialize(n)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    typ = torch.empty(n, dtype=torch.int32, device="cuda")
    fns = [lib.nl_cna, lib.nl_cna_enqueue]
    # no list
    for fn in fns:
        assert fn(nl._h, qd.data_ptr(), 4, 1, 1.0, typ.data_ptr(), None, None, None) == NL_ERR_STATE
    # the arguments come first, before any state
    for fn in fns:
        assert fn(nl._h, qd.data_ptr(), 4, 1, 1.0, None, None, None, None) == NL_ERR_ARG
        assert fn(nl._h, None, 4, 1, 1.0, typ.data_ptr(), None, None, None) == NL_ERR_ARG
        assert fn(None, qd.data_ptr(), 4, 1, 1.0, typ.data_ptr(), None, None, None) == NL_ERR_ARG
        for stride in (0, 2, 5):
            assert fn(nl._h, qd.data_ptr(), stride, 1, 1.0, typ.data_ptr(), None, None, None) == NL_ERR_ARG
        for r in (0.0, -1.0, np.inf, np.nan):
            assert fn(nl._h, qd.data_ptr(), 4, 1, r, typ.data_ptr(), None, None, None) == NL_ERR_ARG
        for mode in (-1, 2, 7):
            assert fn(nl._h, qd.data_ptr(), 4, mode, 1.0, typ.data_ptr(), None, None, None) == NL_ERR_ARG
    nl.update(qd, sync=True)
    builds = nl.update_stats()[1]
    # the reach: rc = 1.69, skin = 0.25 -- 1.4 is within rc - skin = 1.44, 1.5 and 1.69 only within rc, 1.7 within neither
    assert abs(rc - 1.69) < 1e-12
    for r_max, sync_ok, enq_ok in ((1.4, True, True), (1.5, True, False), (rc, True, False), (1.7, False, False)):
        for wait, ok in ((True, sync_ok), (False, enq_ok)):
            for adaptive in MODES:
                if ok:
                    nl.cna(qd, r_max, adaptive=adaptive, wait=wait)
                else:
                    with pytest.raises(NLError) as e:
                        nl.cna(qd, r_max, adaptive=adaptive, wait=wait)
                    assert e.value.code == NL_ERR_ARG, (r_max, wait)
    # a call is no reason to build
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == builds
    # with a type table the reach is the smallest rc_ab > 0: a pair of types with rc_ab = 0 asks for nothing
    types = (np.arange(n) % 3).astype(np.int32)
    nl.set_type_cutoffs(types, [[rc, rc, 0.0], [rc, 1.4, rc], [0.0, rc, rc]])
    nl.MakeNeighList(qd, n)
    nl.cna(qd, 1.4)
    with pytest.raises(NLError) as e:
        nl.cna(qd, 1.5)
    assert e.value.code == NL_ERR_ARG
    # n == 0: the calls succeed and write nothing
    empty = _nl(box6, mask, np.float32, rc)
    empty.Initialize(16)
    empty.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    typ.fill_(7)
    cnt = torch.full((n, 8), 7, dtype=torch.int32, device="cuda")
    sm = torch.full((6,), 7, dtype=torch.int64, device="cuda")
    for fn in fns:
        for mode in (0, 1):
            assert fn(empty._h, qd.data_ptr(), 4, mode, 1.0, typ.data_ptr(), cnt.data_ptr(), sm.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (typ == 7).all() and (cnt == 7).all() and (sm == 7).all()
    # the outputs that are left out, and tensors of the caller
    nl2, qd2 = _built(q, box6, mask, np.float32, rc)
    t, c, s = nl2.cna(qd2, 1.5)
    assert c is None and s.shape == (6,) and s.dtype == torch.int64 and t.shape == (n,) and t.dtype == torch.int32
    t2, c2, s2 = nl2.cna(qd2, 1.5, counts=cnt, summary=False)
    assert c2 is cnt and s2 is None and torch.equal(t, t2) and s.sum() == n + s[5]
    # the Python side's checks
    with pytest.raises(TypeError):
        nl2.cna(qd2, 1.5, counts=torch.zeros((n, 8), dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        nl2.cna(qd2, 1.5, summary=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        nl2.cna(qd2.double(), 1.5)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_on_a_callers_held_stream(dtype):
    """A non-blocking stream of the caller's, held back by a delay: the positions are written behind the delay, and the update
    and both analyses enqueued on that stream read what was written."""
    from tests.stream_util import device, held_stream, rolled

    torch = _torch()
    q = _hot()[0]
    n = len(q)
    nl = _skin_handle(dtype)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    qd = dec.clone()
    counts = [torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in MODES]
    summary = [torch.empty(6, dtype=torch.int64, device="cuda") for _ in MODES]

    def calls():
        return [nl.cna(qd, R_SKIN[a], adaptive=a, counts=counts[k], summary=summary[k], wait=False)[0] for k, a in enumerate(MODES)]

    nl.update(qd, sync=True)  # (warm, on the decoy: nothing allocates on the handle while the stream is held)
    calls()
    torch.cuda.synchronize()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        types = calls()
        h.assert_held(f"cna {np.dtype(dtype).name}")
    nl.synchronize()
    for k, a in enumerate(MODES):
        uc.check(_host(types[k]), _host(counts[k]), _host(summary[k]), _skin_ref(False, a, dtype), ("held", a))

"""Per-axis periodic boundaries (nl_set_periodic_axes): the minimum image on the axes of a mask, the reference's open-box
rule on the others.

The reference for a mixed mask is built only from what exists: oracle.build_pbc (or build_pbc_full), the minimum-image
definition that is itself checked against a brute force (tests/test_oracle.py), run on a PADDED box
    box'[d] = L[d]           on a periodic axis,
    box'[d] = L[d] + 2 rc    on an open axis,
with the positions unchanged and every open-axis coordinate in [0, L + rc/2).  Why this is the list of the mask:
  * No open-axis coordinate is shifted in the padded box (each lies in [0, L') and its cell index never wraps), so the
    open-axis difference of every pair is the raw one, bit for bit -- the open axis's rule.
  * A pair that the padded box could only reach through an open face is at least 2 rc - rc/2 apart there: never
    listed.  The periodic axes keep their box, mesh, images and rounding, so they decide exactly as mask 7 does.
  * The mesh of an open axis differs from the handle's, but a mesh only decides which pairs are visited, never the
    predicate; each side visits every pair within rc.
test_padded_reference_equals_a_brute_force checks the construction itself on the CPU, against an independent numpy
brute force (per-axis minimum image in float64), so that the GPU assertions rest on something independent.
Every GPU list is compared after the reference's canonical sort, bit for bit.
"""
import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.util import canonical_csr, check_lj, lj_list_separations, lj_pair_magnitudes, lj_rows_off_the_band

BOX = (27.0, 24.0, 40.0)  # non-cubic: a mask applied to the wrong axis fails
RC = 3.3
MIXED = (1, 2, 3, 4, 5, 6)


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def padded_box(box, rc, mask):
    return tuple(float(box[d]) if mask >> d & 1 else float(box[d]) + 2.0 * rc for d in range(3))


def reference(q, rc, box, mask, full=False):
    """The list of nl_set_periodic_axes(mask) (module docstring): canonical CSR."""
    po = _po()
    return (po.build_pbc_full if full else po.build_pbc)(q, rc, padded_box(box, rc, mask))


def positions(n, box, rc, mask, dtype, seed):
    """Uniform in the box, plus particles just outside [0, L) on every axis -- below 0 and above L on a periodic axis,
    above L (up to L + rc/2, the reference's range) on an open one -- and particles exactly at 0 and at L."""
    rng = np.random.default_rng(seed)
    L = np.array(box, dtype=np.float64)
    pos = rng.uniform(0.0, 1.0, size=(n, 3)) * L
    k = max(n // 60, 8)
    for d in range(3):
        idx = rng.choice(n, 2 * k + 8, replace=False)
        if mask >> d & 1:
            pos[idx[:k], d] = -rng.uniform(0.0, 0.49 * rc, size=k)
        else:
            pos[idx[:k], d] = L[d] + rng.uniform(0.0, 0.49 * rc, size=k)
        pos[idx[k:2 * k], d] = L[d] + rng.uniform(0.0, 0.49 * rc, size=k)
        pos[idx[2 * k:2 * k + 4], d] = L[d]
        pos[idx[2 * k + 4:], d] = 0.0
    q = np.zeros((n, 4), dtype=dtype)
    q[:, :3] = pos.astype(dtype)
    return q


def brute_force(q, rc, box, mask):
    """O(N^2) float64 numpy: per-axis minimum image on the axes of the mask.  Returns (pairs {(i, j), i < j}, pairs
    within 1e-9 rc of the cut-off, which are left undecided)."""
    p = q[:, :3].astype(np.float64)
    L = np.array(box, dtype=np.float64)
    per = np.array([bool(mask >> d & 1) for d in range(3)])
    keep, edge = set(), set()
    for i in range(len(p) - 1):
        d = p[i + 1:] - p[i]
        d[:, per] -= L[per] * np.round(d[:, per] / L[per])
        r = np.sqrt((d * d).sum(axis=1))
        js = np.arange(i + 1, len(p))
        keep.update((i, int(j)) for j in js[r <= rc])
        edge.update((i, int(j)) for j in js[np.abs(r - rc) <= 1e-9 * rc])
    return keep, edge


def pair_set(kp, lst):
    rows = np.repeat(np.arange(len(kp) - 1), np.diff(kp))
    return set(zip(rows.tolist(), np.asarray(lst).tolist()))


def crosses(q, kp, lst, box, axes):
    """Does the list hold a pair whose raw separation along one of `axes` exceeds half the box (a pair across a face)?"""
    rows = np.repeat(np.arange(len(kp) - 1, dtype=np.int64), np.diff(kp))
    d = np.abs(q[rows, :3].astype(np.float64) - q[np.asarray(lst, dtype=np.int64), :3].astype(np.float64))
    return any(bool((d[:, a] > 0.5 * box[a]).any()) for a in axes)


# ---------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("mask", range(8))
def test_padded_reference_equals_a_brute_force(mask):
    for seed, box, rc, n in ((1, (12.0, 11.0, 14.0), 3.0, 2000), (2, (10.5, 16.0, 9.9), 3.2, 3000)):
        q = positions(n, box, rc, mask, np.float64, seed + 10 * mask)
        ref = reference(q, rc, box, mask)
        got = pair_set(ref.key_pointer, ref.sorted_list)
        want, edge = brute_force(q, rc, box, mask)
        assert got - edge == want - edge, (mask, seed, len(got ^ want))
        assert len(want) > 1000
        per = [d for d in range(3) if mask >> d & 1]
        opn = [d for d in range(3) if not mask >> d & 1]
        if per:
            assert crosses(q, ref.key_pointer, ref.sorted_list, box, per)
        if opn:  # the case has pairs across an open face that the mask must leave out
            full = _po().build_pbc(q, rc, box)
            assert crosses(q, full.key_pointer, full.sorted_list, box, opn)
            assert not crosses(q, ref.key_pointer, ref.sorted_list, box, opn)


def test_axes_forms():
    from md_neighbor_list_amd.neighlist import axes_mask

    assert axes_mask("xy") == 3 and axes_mask("z") == 4 and axes_mask("xyz") == 7 and axes_mask("") == 0
    assert axes_mask((True, False, True)) == 5 and axes_mask([False, True, True]) == 6
    assert axes_mask(True) == 7 and axes_mask(False) == 0 and axes_mask(1) == 7 and axes_mask(0) == 0
    for bad in ("xw", (True, False), "q"):
        with pytest.raises(ValueError):
            axes_mask(bad)


# ---------------------------------------------------------------------------------------------------- GPU


def _handle(rc, box, n, dtype, mask=0, full=False):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full)
    nl.set_periodic(axes=tuple(bool(mask >> d & 1) for d in range(3)))
    nl.Initialize(n)
    return nl


def _list(nl):
    """(key_pointer, canonical list) of the handle's last build."""
    if nl.full_list:
        kp, lst, _ = (t.cpu().numpy() for t in nl.full_csr())
    else:
        kp, lst = nl.key_pointer().cpu().numpy(), nl.sorted_list().cpu().numpy()
    return kp.astype(np.int64), canonical_csr(kp, lst)


def _assert_matches(nl, q, rc, box, mask, what=""):
    ref = reference(q, rc, box, mask, nl.full_list)
    kp, lst = _list(nl)
    assert int(kp[-1]) == len(ref.sorted_list), (what, int(kp[-1]), len(ref.sorted_list))
    assert np.array_equal(kp, ref.key_pointer), what
    assert np.array_equal(lst, ref.sorted_list), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_mask_against_the_padded_reference(dtype):
    torch = _torch()
    n = 20000
    for mask in range(8):
        q = positions(n, BOX, RC, mask, dtype, 100 + mask)
        qd = torch.from_numpy(q).cuda()
        if mask in MIXED:  # the case is not vacuous: pairs across a periodic face, and across an open one if it were
            ref = reference(q, RC, BOX, mask)
            full7 = _po().build_pbc(q, RC, BOX)
            assert crosses(q, ref.key_pointer, ref.sorted_list, BOX, [d for d in range(3) if mask >> d & 1])
            assert crosses(q, full7.key_pointer, full7.sorted_list, BOX, [d for d in range(3) if not mask >> d & 1])
        for full in (False, True):
            nl = _handle(RC, BOX, n, dtype, mask, full)
            assert nl.periodic_mask() == mask
            nl.MakeNeighList(qd, n)
            assert nl.build_info()["masks"]
            _assert_matches(nl, q, RC, BOX, mask, (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("variant,binning", [(v, b) for v in (1, 3) for b in (0, 1)])
def test_build_paths(variant, binning, monkeypatch):
    """NL_SWEEP_VARIANT 1 (COUNT + FILL sweeps) and 3 (hit masks), NL_BINNING 0 (rows) and 1 (atomic rank),
    NL_OFFSET_WIDTH 32 and 64."""
    torch = _torch()
    monkeypatch.setenv("NL_SWEEP_VARIANT", str(variant))
    monkeypatch.setenv("NL_BINNING", str(binning))
    n = 20000
    for width in (32, 64):
        monkeypatch.setenv("NL_OFFSET_WIDTH", str(width))
        for mask in (3, 5):
            q = positions(n, BOX, RC, mask, np.float32, 200 + mask)
            for full in (False, True):
                nl = _handle(RC, BOX, n, np.float32, mask, full)
                nl.MakeNeighList(torch.from_numpy(q).cuda(), n)
                info = nl.build_info()
                assert info["variant"] == variant and info["offset_bits"] == width
                _assert_matches(nl, q, RC, BOX, mask, (mask, full, width))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_box(dtype):
    """~90 particles per cell: the stencil stream takes two LDS batches and the list is expanded by k_fill_dense."""
    torch = _torch()
    n = 60000
    for mask in (3, 5):
        q = positions(n, BOX, RC, mask, dtype, 300 + mask)
        for full in (False, True):
            nl = _handle(RC, BOX, n, dtype, mask, full)
            nl.MakeNeighList(torch.from_numpy(q).cuda(), n)
            assert nl.build_info()["mask_rows"] > 1
            _assert_matches(nl, q, RC, BOX, mask, (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
def test_masks_0_and_7_are_the_existing_modes(dtype, full):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU
    from md_neighbor_list_amd._lib import check

    n = 20000
    q = positions(n, BOX, RC, 0, dtype, 400)
    qd = torch.from_numpy(q).cuda()
    tdt = torch.float32 if dtype == np.float32 else torch.float64

    def run(setup):
        nl = NeighListGPU(RC, *BOX, dtype=tdt, full_list=full)
        nl.Initialize(n)
        setup(nl)
        nl.MakeNeighList(qd, n)
        kp, lst = _list(nl)
        return kp, lst, nl.list_checksum(), nl.build_info()

    for a, b in (
        (run(lambda nl: nl.set_periodic(True)), run(lambda nl: check(nl._lib.nl_set_periodic_axes(nl._h, 7)))),
        (run(lambda nl: nl.set_periodic(True)), run(lambda nl: nl.set_periodic(axes="xyz"))),
        (run(lambda nl: None), run(lambda nl: check(nl._lib.nl_set_periodic_axes(nl._h, 0)))),
        (run(lambda nl: None), run(lambda nl: nl.set_periodic(axes=(False, False, False)))),
    ):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2] == b[2] and a[3] == b[3]


@pytest.mark.gpu
def test_graph_is_keyed_on_the_mask():
    torch = _torch()
    n = 20000
    q = positions(n, BOX, RC, 2, np.float32, 500)  # (open-axis coordinates >= 0 on x and z: valid for masks 3 and 6)
    qd = torch.from_numpy(q).cuda()
    nl = _handle(RC, BOX, n, np.float32, 3)
    nl.set_graph(True)
    for _ in range(3):  # captured, then replayed
        nl.MakeNeighList(qd, n, sync=False)
        nl.synchronize()
    _assert_matches(nl, q, RC, BOX, 3, "mask 3")
    nl.set_periodic(axes="yz")
    assert nl.periodic_mask() == 6
    nl.MakeNeighList(qd, n, sync=False)
    nl.synchronize()
    _assert_matches(nl, q, RC, BOX, 6, "mask 6 after a graph of mask 3")
    assert not np.array_equal(_list(nl)[1], reference(q, RC, BOX, 3).sorted_list)


def _r2(q, snap, box, mask):
    """Rule (c) with the mask: d in the position type, then double; minimum image on the periodic axes only."""
    d = (q[:, :3] - snap[:, :3]).astype(np.float64)
    for a in range(3):
        if mask >> a & 1:
            d[:, a] = d[:, a] - box[a] * np.rint(d[:, a] / box[a])
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_skin_update_folds_the_periodic_axes_only(dtype):
    torch = _torch()
    mask, skin, n = 3, 0.6, 20000
    thr = (0.5 * skin) ** 2
    q0, _ = inputs.uniform_box(n, dtype=dtype, seed=600, box=BOX)
    q0[5, :3] = (BOX[0] - 0.05, 10.0, 10.0)
    q0[6, :3] = (10.0, 10.0, 0.05)
    seq = [q0]
    q = q0.copy()
    q[5, 0] = 0.05  # across the periodic x face: 0.1 by the minimum image -> no build
    seq.append(q.copy())
    q[7, 2] = q[7, 2] + (0.4 if q[7, 2] < 20.0 else -0.4)  # 0.4 > skin/2 along z -> build
    seq.append(q.copy())
    q[8, 1] = q[8, 1] + (0.1 if q[8, 1] < 12.0 else -0.1)  # small move -> no build
    seq.append(q.copy())
    q[6, 2] = BOX[2] - 0.05  # across the OPEN z face: 0.1 by an image, L - 0.1 as given -> build
    seq.append(q.copy())
    nl = _handle(RC, BOX, n, dtype, mask)
    nl.set_skin(skin)
    qd = torch.from_numpy(seq[0]).cuda()
    nl.update(qd, sync=True)
    _assert_matches(nl, seq[0], RC, BOX, mask, "first update")
    snap, builds, expect = seq[0], 1, [False, True, False, True]
    for k in range(1, len(seq)):
        qd.copy_(torch.from_numpy(seq[k]))
        nl.update(qd, sync=True)
        r2 = _r2(seq[k], snap, BOX, mask)
        build = bool(np.isnan(r2).any() or r2.max() > thr)
        assert build == expect[k - 1], k
        if build:
            snap, builds = seq[k], builds + 1
        assert nl.update_stats() == (k + 1, builds), k
        _assert_matches(nl, snap, RC, BOX, mask, ("update", k))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("mask", [3, 4])
def test_lj_forces_fold_per_axis(mask, full, dtype):
    """nl_lj_forces on a mixed-mask list against float64 numpy on the reference list, each component folded only on
    its periodic axis; tolerance 2e-4 (fp32) / 1e-11 (fp64) of the largest component; the total force vanishes."""
    torch = _torch()
    rc, box = 3.0, (32.0, 30.0, 34.0)
    q, _ = inputs.uniform_box(30000, dtype=dtype, seed=61 + mask, box=box)

    def pairs(q):
        ref = reference(q, rc, box, mask)
        rows = np.repeat(np.arange(len(q), dtype=np.int64), np.diff(ref.key_pointer))
        cols = ref.sorted_list.astype(np.int64)
        raw = q[rows, :3].astype(np.float64) - q[cols, :3].astype(np.float64)
        d = lj_list_separations(q, rows, cols, (*box, 0.0, 0.0, 0.0), mask)  # (folded before it is rounded to float64)
        return rows, cols, raw, d, (d * d).sum(axis=1)

    # no pair closer than 0.8 sigma (a well-conditioned reference sum in fp32, finite forces): drop such particles
    rows, cols, raw, d, r2 = pairs(q)
    close = np.zeros(len(q), dtype=bool)
    close[rows[r2 <= 0.64]] = True
    close[cols[r2 <= 0.64]] = True
    q = np.ascontiguousarray(q[~close])
    n = len(q)
    rows, cols, raw, d, r2 = pairs(q)
    assert r2.min() > 0.64
    for a in range(3):
        if mask >> a & 1:
            assert (np.abs(raw[:, a]) > 0.5 * box[a]).any()  # pairs across this periodic face enter the forces
    s6 = (1.0 / r2) ** 3
    fr = 24.0 * (2.0 * s6 * s6 - s6) / r2
    want = np.zeros((n, 4))
    for c in range(3):
        np.add.at(want[:, c], rows, fr * d[:, c])
        np.add.at(want[:, c], cols, -fr * d[:, c])
    pe = 4.0 * (s6 * s6 - s6)
    np.add.at(want[:, 3], rows, 0.5 * pe)
    np.add.at(want[:, 3], cols, 0.5 * pe)

    nl = _handle(rc, box, n, dtype, mask, full)
    qd = torch.from_numpy(q).cuda()
    nl.MakeNeighList(qd, n)
    got = nl.lj_forces(qd, 1.0, 1.0).cpu().numpy().astype(np.float64)
    scale = np.abs(want).max(axis=0)
    tol = 2e-4 if dtype == np.float32 else 1e-11
    assert np.all(np.abs(got - want) <= tol * scale), (np.abs(got - want) / scale).max(axis=0)
    # and per particle and component within c u S (tests/test_lj_consumer.py), off the 64-ulp band of rc_force = rc
    check_lj(got, want, lj_pair_magnitudes(n, rows, cols, d, r2), dtype, rows=lj_rows_off_the_band(n, rows, cols, r2, rc, dtype))
    total = got[:, :3].sum(axis=0)
    assert np.all(np.abs(total) <= (1e-4 if dtype == np.float32 else 1e-10) * np.abs(got[:, :3]).sum(axis=0)), total


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [3, 4])
def test_slabs_union_is_the_reference(mask):
    """Three slabs of the box in one process (fp32): the union of their rows is the mask's list.  z open (mask 3): the
    box-end ranks' ghost layers hold no partner of a particle in [0, L), so sending them empty gives the same rows."""
    torch = _torch()
    from md_neighbor_list_amd import slab

    q, _ = inputs.uniform_box(42000, dtype=np.float32, seed=700 + mask, box=BOX)
    mz = int(BOX[2] / RC)
    iz = slab.z_layer(torch.from_numpy(q), BOX, RC).numpy()
    ref = reference(q, RC, BOX, mask)
    for empty_end_ghosts in ((False, True) if mask == 3 else (False,)):
        rows = {}
        for z_lo, z_hi in ((0, 4), (4, 8), (8, mz)):
            own = np.nonzero((iz >= z_lo) & (iz < z_hi))[0]
            glo = np.nonzero(iz == (z_lo - 1) % mz)[0]
            ghi = np.nonzero(iz == z_hi % mz)[0]
            if empty_end_ghosts:
                glo = glo[:0] if z_lo == 0 else glo
                ghi = ghi[:0] if z_hi == mz else ghi
            order = np.concatenate([own, glo, ghi])
            nl = _handle(RC, BOX, len(order), np.float32, mask)
            nl.MakeNeighListSlab(torch.from_numpy(q[order]).cuda(), torch.from_numpy(order.astype(np.int32)).cuda(),
                                 len(own), z_lo, z_hi, sync=True)
            kp, sl = nl.key_pointer().cpu().numpy(), nl.sorted_list().cpu().numpy()
            for r, g in enumerate(own):
                rows[int(g)] = np.sort(sl[kp[r]:kp[r + 1]])
        assert sorted(rows) == list(range(len(q)))
        got = np.concatenate([rows[i] for i in range(len(q))])
        counts = np.array([len(rows[i]) for i in range(len(q))])
        assert np.array_equal(counts, ref.number_of_partners), empty_end_ghosts
        assert np.array_equal(got, ref.sorted_list), empty_end_ghosts


@pytest.mark.gpu
def test_mask_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NLError, check

    nl = _handle(RC, BOX, 1000, np.float32)
    assert nl.periodic_mask() == 0 and nl.periodic_axes == (False, False, False) and not nl.minimum_image
    for bad in (-1, 8):
        with pytest.raises(NLError) as e:
            check(nl._lib.nl_set_periodic_axes(nl._h, bad))
        assert e.value.code == NL_ERR_ARG
        assert nl.periodic_mask() == 0
    for m in range(8):
        check(nl._lib.nl_set_periodic_axes(nl._h, m))
        assert nl.periodic_mask() == m
    nl.set_periodic(axes="xz")
    assert nl.periodic_mask() == 5 and nl.periodic_axes == (True, False, True) and not nl.minimum_image
    nl.set_periodic(True)
    assert nl.periodic_mask() == 7 and nl.periodic_axes == (True, True, True) and nl.minimum_image
    nl.set_periodic(False)
    assert nl.periodic_mask() == 0 and not nl.minimum_image
    from md_neighbor_list_amd import NeighListGPU

    h = NeighListGPU(RC, *BOX, minimum_image="xy")
    assert h.periodic_mask() == 3 and h.periodic_axes == (True, True, False) and not h.minimum_image

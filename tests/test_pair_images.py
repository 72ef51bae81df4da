"""The periodic image of every entry of the list (nl_set_pair_images, nl_get_pair_images, nl_pair_vectors).

The rule of include/nl_hip.h, s = n_j + w_ij - n_i, is restated here in numpy from the binning of tests/test_triclinic_box.py
(`bin_frame`, whose wraps are restated in `wraps_of`) and checked against an independent float64 reference: with
lambda = (q_j - q_i) H^-1 the image is s_ref = -rint(lambda) on the periodic axes and 0 on the open ones.  The reference is
unambiguous: a pair within rc has |lambda_d + s_d| <= rc / w_d <= 1/3 (every axis holds three cells of at least rc).
Every GPU image is compared with s_ref entry by entry, and every GPU list with the replay of the rule, bit for bit.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_triclinic_box import BOX, RC, bin_frame, lattice, mesh_of, positions, replay_pairs, shear_of, tilted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nl_set_pair_images", "nl_get_pair_images", "nl_pair_vectors", "nl_pair_vectors_enqueue")
# (mask, tilt) of the image tests; "none" = the orthogonal box
CASES = [(7, "none"), (7, "xy"), (7, "all"), (7, "neg"), (7, "half"), (3, "half"), (5, "none"), (0, "none")]


def box_of(mask, tilt):
    return BOX + (0.0, 0.0, 0.0) if tilt == "none" else tilted(tilt, mask)


# ------------------------------------------------------------------------------------------------------ the rule
def wraps_of(q, rc, box, mask, T):
    """n_p: the wraps local_cell decides from the input coordinate (+1: the cell index was below 0 and the particle is
    stored one box vector up; -1: the other way round; 0 on an open axis).  The lines of bin_frame that it does not return."""
    x = q[:, :3].astype(T)
    m = mesh_of(rc, box)
    kxy, kxz, kyz = shear_of(box, T)
    xs, ys = x[:, 0], x[:, 1]
    if any(float(v) != 0.0 for v in box[3:]):
        xs = (x[:, 0] - x[:, 1] * kxy) - x[:, 2] * kxz
        ys = x[:, 1] - x[:, 2] * kyz
    sheared = (xs, ys, x[:, 2])
    wrap = np.zeros((len(q), 3), dtype=np.int64)
    for d in range(3):
        if not mask >> d & 1:
            continue
        ms = float(box[d]) / m[d]
        ims = T(1.0 / float(np.float32(ms))) if T == np.float32 else T(1.0 / ms)
        t = sheared[d] * ims
        v = np.trunc(t).astype(np.int64)
        v -= ((t < 0) & (v.astype(T) != t)).astype(np.int64)
        wrap[:, d] = np.where(v < 0, 1, np.where(v >= m[d], -1, 0))
    return wrap


def image_rule(q, rc, box, mask, T, rows, parts):
    """s = n_j + w_ij - n_i for the entries (rows, parts)."""
    box = tuple(float(v) for v in box)
    _pos, cells, bad = bin_frame(q, rc, box, mask, T)
    assert not bad.any()
    m = mesh_of(rc, box)
    n = wraps_of(q, rc, box, mask, T)
    w = np.zeros((len(rows), 3), dtype=np.int64)
    for d in range(3):
        if mask >> d & 1:
            ci, cj = cells[rows, d], cells[parts, d]
            w[:, d] = np.where((ci == 0) & (cj == m[d] - 1), -1, np.where((ci == m[d] - 1) & (cj == 0), 1, 0))
    return n[parts] + w - n[rows]


def image_ref(q, box, mask, rows, parts):
    """(s_ref, lambda): the independent float64 reference."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    H = np.array([[Lx, 0.0, 0.0], [xy, Ly, 0.0], [xz, yz, Lz]])
    p = q[:, :3].astype(np.float64)
    lam = (p[parts] - p[rows]) @ np.linalg.inv(H)
    s = -np.rint(lam).astype(np.int64)
    for d in range(3):
        if not mask >> d & 1:
            s[:, d] = 0
    return s, lam


def pair_vectors_ref(q, box, T, rows, parts, s):
    """{dx, dy, dz, r2} of nl_pair_vectors, bit for bit: S(s) in double in lattice()'s order, rounded to T once, added where
    it is not 0, then q_j' - q_i and r2 = (dx^2 + dy^2) + dz^2, every operation in T."""
    x = q[:, :3].astype(T)
    S = lattice(tuple(float(v) for v in box), s)
    St = S.astype(T)
    out = np.zeros((len(rows), 4), dtype=T)
    for d in range(3):
        pj = np.where(S[:, d] == 0.0, x[parts, d], x[parts, d] + St[:, d])
        out[:, d] = pj - x[rows, d]
    out[:, 3] = (out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2]
    return out


def same_bits(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


# ------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask,tilt", CASES + [(3, "none")])
def test_rule_equals_the_float64_reference(dtype, mask, tilt):
    box = box_of(mask, tilt)
    q = positions(3000, RC, box, mask, dtype, seed=7)
    counts = {}
    for full in (False, True):
        rows, parts, _n = replay_pairs(q, RC, box, mask, dtype, full)
        s = image_rule(q, RC, box, mask, dtype, rows, parts)
        s_ref, lam = image_ref(q, box, mask, rows, parts)
        assert int((s != s_ref).any(axis=1).sum()) == 0
        assert np.abs(s).max() <= 3
        per = [d for d in range(3) if mask >> d & 1]
        if per:
            assert np.abs(lam + s_ref)[:, per].max() <= 1.0 / 3.0  # the reference is unambiguous
            assert (s != 0).any(axis=1).mean() > 0.1  # (returning zeros does not pass)
        else:
            assert not s.any()
        counts[full] = len(rows)
        if full:  # the two rows of a pair: exactly antisymmetric
            key = rows * len(q) + parts
            order = np.argsort(key)
            at = np.searchsorted(key[order], parts * len(q) + rows)
            assert np.array_equal(key[order][at], parts * len(q) + rows)
            assert np.array_equal(s[order][at], -s)
    assert counts[True] == 2 * counts[False] > 20000  # no missing reverses on these seeds


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pair_vectors_restatement_is_the_displacement(dtype):
    box = box_of(7, "all")
    q = positions(3000, RC, box, 7, dtype, seed=7)
    rows, parts, _n = replay_pairs(q, RC, box, 7, dtype)
    s = image_rule(q, RC, box, 7, dtype, rows, parts)
    v = pair_vectors_ref(q, box, dtype, rows, parts, s)
    p = q[:, :3].astype(np.float64)
    want = p[parts] + lattice(box, s) - p[rows]
    tol = 64 * np.finfo(dtype).eps * max(BOX)  # roundings of coordinates of up to ~1.5 box lengths
    assert np.abs(v[:, :3].astype(np.float64) - want).max() <= tol
    assert np.sqrt(v[:, 3].astype(np.float64)).max() <= RC * (1 + 1e-5)  # (at these images every pair is within rc)


def test_header_declares_and_python_binds_the_entry_points():
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd.neighlist import NeighListGPU

    with open(os.path.join(ROOT, "include", "nl_hip.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(nl_handle_t h" % name, hdr, re.M), name
        assert name in _lib.PROTOTYPES, name
    assert "s = n_j + w_ij - n_i" in hdr
    for method in ("set_pair_images", "pair_images", "pair_vectors", "edge_index"):
        assert callable(getattr(NeighListGPU, method, None)), method


def test_entry_count_is_the_library_s_not_twice_the_pairs():
    """The two rows of a full list decide a pair on their own (within one ulp of rc across a periodic face they may differ),
    so a full list can hold an odd number of entries: list_entries() must be the count nl_get_full_csr / nl_get_half_csr
    report, never 2 x nl_number_of_pairs (which rounds an odd total down).  pair_vectors() sizes and checks its output by
    the nentries of nl_get_pair_images, the same number (the GPU tests compare the two)."""
    from md_neighbor_list_amd.neighlist import NeighListGPU

    class Lib:  # the three getters as the C ABI answers them for a full list of 7 entries / a half list of 5
        def __init__(self, entries):
            self.entries = entries

        def _csr(self, h, kp, sl, nop, ne):
            ne._obj.value = self.entries
            return 0

        nl_get_full_csr = nl_get_full_csr64 = nl_get_half_csr = nl_get_half_csr64 = _csr

        def nl_number_of_pairs(self, h, npairs):
            npairs._obj.value = self.entries // 2
            return 0

    for full, entries in ((True, 7), (True, 8), (False, 5)):
        nl = object.__new__(NeighListGPU)
        nl._lib, nl._h, nl.full_list = Lib(entries), None, full
        assert nl.list_entries() == entries


# ------------------------------------------------------------------------------------------------------- GPU tests
def _torch():
    import torch

    return torch


def _handle(box, dtype, mask, n, full=False, images=True, **kw):
    from tests.test_triclinic_box import _handle as handle

    nl = handle(box, dtype, mask, n, full=full, **kw)
    if images:
        nl.set_pair_images(True)
    return nl


def _build(nl, q, sync=True):
    torch = _torch()
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(qd, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return qd


def _entries(nl):
    """(rows, partners, images) of the last build, in the list's own order."""
    ei = nl.edge_index().cpu().numpy()
    img = nl.pair_images().cpu().numpy()
    assert img.dtype == np.int8 and img.shape == (ei.shape[1], 3)
    return ei[0], ei[1], img.astype(np.int64)


def _same_pairs(rows, parts, want_rows, want_parts, n):
    return np.array_equal(np.sort(rows * n + parts), np.sort(want_rows * n + want_parts))


def _check_images(nl, q, box, mask, dtype, full=False, rc=RC, replayed=True):
    """The list is the replay's, and every image is the reference's.  Returns (rows, partners, images)."""
    rows, parts, img = _entries(nl)
    if replayed:
        wr, wp, n = replay_pairs(q, rc, box, mask, dtype, full)
        assert _same_pairs(rows, parts, wr, wp, n)
    s_ref, _lam = image_ref(q, box, mask, rows, parts)
    bad = int((img != s_ref).any(axis=1).sum())
    assert bad == 0, f"{bad} of {len(rows)} images differ"
    assert len(rows) > 1000
    return rows, parts, img


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("mask,tilt", CASES)
def test_images_equal_the_reference(dtype, full, mask, tilt):
    box = box_of(mask, tilt)
    q = positions(8000, RC, box, mask, dtype, seed=3)
    nl = _handle(box, dtype, mask, len(q), full=full)
    _build(nl, q)
    _rows, _parts, img = _check_images(nl, q, box, mask, dtype, full)
    if mask == 0:
        assert not img.any()
    else:
        assert (img != 0).any(axis=1).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("mask,tilt", [(7, "none"), (7, "all"), (3, "half")])
def test_images_where_no_particle_is_wrapped(dtype, full, mask, tilt):
    # every particle inside the box: the stage then skips the partner of rows whose cell touches no periodic face
    box = box_of(mask, tilt)
    rng = np.random.default_rng(19)
    lam = rng.uniform(1e-5, 1.0 - 1e-5, size=(8000, 3))
    if tilt == "none":
        lam[:50, 0] = 0.0
    q = np.zeros((8000, 4), dtype=dtype)
    q[:, :3] = (lam @ np.array([[box[0], 0, 0], [box[3], box[1], 0], [box[4], box[5], box[2]]])).astype(dtype)
    nl = _handle(box, dtype, mask, len(q), full=full)
    _build(nl, q)
    _rows, _parts, img = _check_images(nl, q, box, mask, dtype, full)
    assert (img != 0).any(axis=1).mean() > 0.1
    # and a build of wrapped particles on the same handle behind it
    q2 = positions(8000, RC, box, mask, dtype, seed=20)
    _build(nl, q2)
    _check_images(nl, q2, box, mask, dtype, full)
    _build(nl, q)
    _check_images(nl, q, box, mask, dtype, full)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask,tilt", [(7, "all"), (7, "none"), (3, "half")])
def test_full_list_images_are_antisymmetric(dtype, mask, tilt):
    box = box_of(mask, tilt)
    q = positions(8000, RC, box, mask, dtype, seed=4)
    nl = _handle(box, dtype, mask, len(q), full=True)
    _build(nl, q)
    rows, parts, img = _entries(nl)
    n = len(q)
    key = rows * n + parts
    order = np.argsort(key)
    rev = parts * n + rows
    at = np.minimum(np.searchsorted(key[order], rev), len(key) - 1)
    found = key[order][at] == rev  # (the two rows decide on their own: a pair within one ulp of rc may lack its reverse)
    assert (~found).sum() * 10**4 < len(key)
    assert np.array_equal(img[order][at][found], -img[found])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [3, 4])
def test_pair_vectors_bit_for_bit(dtype, stride):
    torch = _torch()
    full = stride == 3
    box = box_of(7, "all")
    q = positions(8000, RC, box, 7, dtype, seed=5)
    qs = np.ascontiguousarray(q[:, :stride])
    nl = _handle(box, dtype, 7, len(q), full=full)
    nl.set_skin(0.4)
    qd = torch.from_numpy(qs).cuda()
    nl.update(qd, sync=True)
    rows, parts, img = _check_images(nl, q, box, 7, dtype, full)
    got = nl.pair_vectors(qd).cpu().numpy()
    assert same_bits(got, pair_vectors_ref(q, box, dtype, rows, parts, img))
    # positions moved by less than skin / 2: the update skips, the images hold, the vectors follow the positions
    rng = np.random.default_rng(6)
    moved = qs.copy()
    moved[:, :3] += rng.uniform(-0.1, 0.1, size=(len(q), 3)).astype(dtype)
    builds = nl.update_stats()[1]
    qd.copy_(torch.from_numpy(moved))
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == builds
    r2, p2, i2 = _entries(nl)
    assert np.array_equal(r2, rows) and np.array_equal(p2, parts) and np.array_equal(i2, img)
    want = pair_vectors_ref(moved, box, dtype, rows, parts, img)
    assert same_bits(nl.pair_vectors(qd).cpu().numpy(), want)
    # the stream-ordered variant behind an update, into a buffer of the list's capacity
    cap = len(rows) + 4096
    nl.set_capacity(cap)
    nl.update(qd, sync=True)
    rows, parts, img = _entries(nl)
    out = torch.zeros((cap, 4), dtype=qd.dtype, device="cuda")
    nl.update(qd)
    nl.pair_vectors(qd, out=out, wait=False)
    nl.synchronize()
    torch.cuda.synchronize()
    assert same_bits(out[:len(rows)].cpu().numpy(), pair_vectors_ref(moved, box, dtype, rows, parts, img))
    assert not out[len(rows):].any()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [("NL_SWEEP_VARIANT", "1"), ("NL_ROWS", "4"), ("NL_IDCLASS", "0"), ("NL_BINNING", "1"),
                                 ("NL_BIN_BUCKETS", "0")])
def test_images_on_the_other_search_paths(env, monkeypatch):
    from md_neighbor_list_amd import inputs

    monkeypatch.setenv(*env)
    box = box_of(7, "half")
    q = positions(8000, RC, box, 7, np.float32, seed=8)
    nl = _handle(box, np.float32, 7, len(q))
    _build(nl, q)
    _check_images(nl, q, box, 7, np.float32)
    # the open box, where the fine rows and the id classes live
    if env[0] == "NL_ROWS":
        q0, b0 = inputs.uniform_box(40000, dtype=np.float32, seed=5, box=(33.0, 33.0, 33.9))
        box0 = tuple(b0) + (0.0, 0.0, 0.0)
    else:
        box0 = box_of(0, "none")
        q0 = positions(8000, RC, box0, 0, np.float32, seed=9)
    nl0 = _handle(box0, np.float32, 0, len(q0))
    _build(nl0, q0)
    _rows, _parts, img = _check_images(nl0, q0, box0, 0, np.float32)
    assert not img.any()
    if env[0] == "NL_ROWS":
        assert nl0.build_info()["fine_rows"] > 0


@pytest.mark.gpu
def test_images_with_64_bit_offsets():
    box = box_of(7, "all")
    q = positions(8000, RC, box, 7, np.float32, seed=10)
    for full in (False, True):
        nl = _handle(box, np.float32, 7, len(q), full=full)
        nl.set_offset_width(64)
        _build(nl, q)
        assert nl.build_info()["offset_bits"] == 64
        rows, parts, img = _check_images(nl, q, box, 7, np.float32, full)
        qd = _torch().from_numpy(q).cuda()
        for dtype in (np.float32, np.float64):  # the consumer behind int64 offsets, both position types
            if dtype == np.float64:
                nl = _handle(box, dtype, 7, len(q), full=full)
                nl.set_offset_width(64)
                qd = _build(nl, q.astype(dtype))
                assert nl.build_info()["offset_bits"] == 64
                rows, parts, img = _check_images(nl, q.astype(dtype), box, 7, dtype, full)
            assert nl.list_entries() == len(rows)
            assert same_bits(nl.pair_vectors(qd).cpu().numpy(), pair_vectors_ref(q.astype(dtype), box, dtype, rows, parts, img))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_images_of_a_dense_box(dtype):
    rc = 4.0
    box = (16.4, 16.2, 16.8, 3.0, 0.0, 0.0)  # 4 x 4 x 4 cells of ~62 particles: several LDS batches a stencil
    assert mesh_of(rc, box) == (4, 4, 4)
    q = positions(4000, rc, box, 7, dtype, seed=11)
    nl = _handle(box, dtype, 7, len(q), rc=rc)
    _build(nl, q)
    assert nl.build_info()["mask_rows"] > 1, nl.build_info()  # k_fill_dense
    _check_images(nl, q, box, 7, dtype, rc=rc)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_images_line_up_with_the_filtered_list(full):
    box = box_of(7, "all")
    n = 8000
    q = positions(n, RC, box, 7, np.float32, seed=12)
    wr, wp, _n = replay_pairs(q, RC, box, 7, np.float32, full)
    excl = np.stack([wr[::3], wp[::3]], axis=1)
    types = (np.arange(n) % 2).astype(np.int32)
    rcm = np.array([[RC, 2.5], [2.5, RC]])
    nl = _handle(box, np.float32, 7, n, full=full)
    nl.set_exclusions(excl, n)
    nl.set_type_cutoffs(types, rcm)
    _build(nl, q)
    rows, parts, _img = _check_images(nl, q, box, 7, np.float32, full, replayed=False)
    got = set((rows * n + parts).tolist())
    assert len(got) == len(rows) and got <= set((wr * n + wp).tolist())
    gone = set((excl[:, 0] * n + excl[:, 1]).tolist()) | set((excl[:, 1] * n + excl[:, 0]).tolist())
    assert not got & gone
    d = q[parts, :3].astype(np.float64) + lattice(box, _img) - q[rows, :3].astype(np.float64)
    far = np.sqrt((d * d).sum(axis=1)) > 2.5 * (1 + 1e-5)
    assert not (far & (types[rows] != types[parts])).any()  # the type table has cut them
    assert 0.2 * len(wr) < len(rows) < 0.7 * len(wr)


@pytest.mark.gpu
def test_growth_grows_the_images():
    box = box_of(7, "all")
    q = positions(8000, RC, box, 7, np.float32, seed=13)
    for tables in (False, True):
        nl = _handle(box, np.float32, 7, len(q))
        nl.set_capacity(1000)
        if tables:
            nl.set_type_cutoffs(np.zeros(len(q), dtype=np.int32), np.array([[RC]]))
        _build(nl, q)  # (synchronous: grows the list, the unfiltered one and the images)
        _check_images(nl, q, box, 7, np.float32)


@pytest.mark.gpu
def test_updates_and_rewraps():
    torch = _torch()
    box = box_of(7, "all")
    dtype = np.float32
    q = positions(8000, RC, box, 7, dtype, seed=14)
    lam = q[:, :3].astype(np.float64) @ np.linalg.inv(np.array([[box[0], 0, 0], [box[3], box[1], 0], [box[4], box[5], box[2]]]))
    inside = int(np.flatnonzero(((lam > 0.3) & (lam < 0.7)).all(axis=1))[0])
    for images in (True, False):
        nl = _handle(box, dtype, 7, len(q), images=images)
        nl.set_skin(0.4)
        qd = torch.from_numpy(q).cuda()
        nl.update(qd, sync=True)
        builds = nl.update_stats()[1]
        if images:
            before = nl.pair_images().clone()
            ptr = nl.pair_images().data_ptr()
            nl.update(qd, sync=True)  # skipped: the list and the images stay
            assert nl.update_stats()[1] == builds
            assert nl.pair_images().data_ptr() == ptr and torch.equal(nl.pair_images(), before)
        # the caller wraps one particle by a box vector: the folded rule (c) does not see it, the unfolded one does
        moved = q.copy()
        moved[inside, :3] += np.array([box[0], 0.0, 0.0], dtype=dtype)
        qd.copy_(torch.from_numpy(moved))
        nl.update(qd, sync=True)
        assert nl.update_stats()[1] == builds + (1 if images else 0)
        if images:
            rows, parts, img = _check_images(nl, moved, box, 7, dtype)
            assert (img[rows == inside][:, 0] == 1).all() and (rows == inside).any()  # (S(s) follows the particle up by a)


@pytest.mark.gpu
def test_graph_replays_and_toggling():
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    torch = _torch()
    box = box_of(7, "half")
    q = positions(8000, RC, box, 7, np.float32, seed=15)
    nl = _handle(box, np.float32, 7, len(q))
    nl.set_graph(True)
    qd = torch.from_numpy(q).cuda()
    first = None
    for _step in range(3):
        nl.MakeNeighList(qd, len(q), sync=False)
        nl.synchronize()
        rows, parts, img = _check_images(nl, q, box, 7, np.float32)
        key = np.argsort(rows * len(q) + parts)
        if first is None:
            first = img[key]
        assert np.array_equal(img[key], first)
    nl.set_pair_images(False)  # another graph: no image stage
    nl.MakeNeighList(qd, len(q), sync=False)
    nl.synchronize()
    with pytest.raises(NLError) as e:
        nl.pair_images()
    assert e.value.code == NL_ERR_STATE
    nl.set_pair_images(True)
    with pytest.raises(NLError) as e:  # the flag dropped the list
        nl.pair_images()
    assert e.value.code == NL_ERR_STATE
    for _step in range(2):
        nl.MakeNeighList(qd, len(q), sync=False)
        nl.synchronize()
        _check_images(nl, q, box, 7, np.float32)
    # graph replays of updates
    nl.set_skin(0.4)
    nl.update(qd, sync=True)
    for _step in range(2):
        nl.update(qd)
        nl.synchronize()
        _check_images(nl, q, box, 7, np.float32)


@pytest.mark.gpu
def test_images_follow_set_box():
    box = box_of(7, "xy")
    q = positions(8000, RC, box, 7, np.float64, seed=16)
    nl = _handle(box, np.float64, 7, len(q))
    _build(nl, q)
    _check_images(nl, q, box, 7, np.float64)
    box2 = box_of(7, "all")
    q2 = positions(8000, RC, box2, 7, np.float64, seed=17)
    nl.set_box(*box2)
    _build(nl, q2)
    _check_images(nl, q2, box2, 7, np.float64)
    qd = _torch().from_numpy(q2).cuda()
    rows, parts, img = _entries(nl)
    assert same_bits(nl.pair_vectors(qd).cpu().numpy(), pair_vectors_ref(q2, box2, np.float64, rows, parts, img))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_enqueued_vectors_of_a_failed_build_are_nan(dtype):
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    box = box_of(7, "all")
    q = positions(8000, RC, box, 7, dtype, seed=21)
    nl = _handle(box, dtype, 7, len(q))
    nl.set_skin(0.4)
    cap = 1000
    nl.set_capacity(cap)
    qd = torch.from_numpy(q).cuda()
    out = torch.zeros((cap, 4), dtype=qd.dtype, device="cuda")
    nl.update(qd)  # asynchronous: the list overflows its capacity and cannot grow
    nl.pair_vectors(qd, out=out, wait=False)  # stream-ordered behind the failed build: NaN, within the capacity
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert torch.isnan(out).all()


@pytest.mark.gpu
def test_errors():
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError, load

    torch = _torch()
    box = box_of(7, "none")
    n = 4000
    q = positions(n, RC, box, 7, np.float32, seed=18)
    nl = _handle(box, np.float32, 7, n, images=False)
    qd = _build(nl, q)
    out = torch.empty((nl.list_entries(), 4), dtype=torch.float32, device="cuda")
    empty = torch.empty((0, 4), dtype=torch.float32, device="cuda")
    for call in (nl.pair_images, lambda: nl.pair_vectors(qd), lambda: nl.pair_vectors(qd, out=out, wait=False),
                 lambda: nl.pair_vectors(qd, out=empty)):
        with pytest.raises(NLError) as e:  # the flag is off
            call()
        assert e.value.code == NL_ERR_STATE
    nl.set_pair_images(True)
    with pytest.raises(NLError) as e:  # no build since
        nl.pair_images()
    assert e.value.code == NL_ERR_STATE
    with pytest.raises(NLError) as e:  # slab builds have no images
        nl.MakeNeighListSlab(qd, torch.arange(n, dtype=torch.int32, device="cuda"), n, 0, nl.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    with pytest.raises(NLError) as e:
        nl.MakeNeighListSlabBegin(qd, None, n, 0, 0, nl.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    assert load().nl_make_list_distributed(nl._h, C.c_void_p(1), qd.data_ptr(), n, n, None, 1) == NL_ERR_STATE
    nl.MakeNeighList(qd, n, sync=False)
    with pytest.raises(NLError) as e:  # a plain asynchronous build may still need the host to complete it
        nl.pair_vectors(qd, out=out, wait=False)
    assert e.value.code == NL_ERR_STATE
    nl.synchronize()
    _check_images(nl, q, box, 7, np.float32)
    nl.pair_vectors(qd, out=out, wait=False)  # (behind a build that has been synchronised)
    torch.cuda.synchronize()
    rows, parts, img = _entries(nl)
    assert same_bits(out.cpu().numpy(), pair_vectors_ref(q, box, np.float32, rows, parts, img))

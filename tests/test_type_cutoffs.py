"""Per-type cut-offs (nl_set_type_cutoffs): a build with a type table keeps an entry (row i, partner j) of the plain list
iff !(r2 > rc2[t_i][t_j]), with r2 the value the search tested and rc2 rounded as the handle's rc is.

The reference (`type_filter`) takes the oracle's list at the handle's rc (pyoracle.build, or the padded-box construction
of tests/test_periodic_axes.py for periodic masks) and replays r2 in the position type with numpy: each particle at the
image the binning stores it at (the cell hash of local_cell, the -+L shift of a wrapped cell on a periodic axis), the
partner shifted across the periodic face through which the row's stencil reaches it.  A CPU test checks that filter
against a float64 brute force over all pairs.  Every GPU list is compared with it after the canonical sort, bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.test_exclusions import _checksum, full_from_half, mixed_pairs, ref_list, remove_pairs
from tests.test_periodic_axes import positions
from tests.util import (ROOT, canonical_csr, check_lj, golden_names, lj_list_separations, lj_pair_magnitudes,
                        lj_rows_off_the_band, load_golden)

BOX = (27.0, 24.0, 40.0)
RC = 3.3


def _torch():
    import torch

    return torch


# ------------------------------------------------------------------------------------------------- numpy reference
def floor_to(v, dtype):
    """The largest value of dtype <= v (a float64)."""
    f = dtype(v)
    if float(f) > v:
        f = np.nextafter(f, dtype(-np.inf))
    return f


def rc2_table(rcm, dtype):
    rcm = np.asarray(rcm, dtype=np.float64)
    return np.array([[floor_to(float(r) * float(r), dtype) for r in row] for row in rcm], dtype=dtype)


def stored_frame(q, rc, box, mask, dtype):
    """(positions at the image the binning stores, cell index per axis) -- local_cell of nl_kernels.hpp in numpy."""
    T = dtype
    x = q[:, :3].astype(T)
    out = x.copy()
    cells = np.zeros((len(q), 3), dtype=np.int64)
    for d in range(3):
        m = int(box[d] / rc)
        ms = box[d] / m
        ims = T(1.0 / float(np.float32(ms))) if T == np.float32 else T(1.0 / ms)
        L = T(box[d])
        t = x[:, d] * ims
        v = np.trunc(t).astype(np.int64)
        per = bool(mask >> d & 1)
        if per:
            v -= ((t < 0) & (v.astype(T) != t)).astype(np.int64)
        sh = np.zeros(len(q), dtype=T)
        lo, hi = v < 0, v >= m
        v[lo] += m
        v[hi] -= m
        sh[lo], sh[hi] = L, -L
        if per:
            out[:, d] = x[:, d] + sh
        cells[:, d] = v
    return out, cells


def entry_r2(q, rc, box, mask, dtype, rows, cols):
    """r2 of the entries (rows[k], cols[k]) as the search tests it, in dtype."""
    T = dtype
    p, c = stored_frame(q, rc, box, mask, dtype)
    pj = p[cols].copy()
    for d in range(3):
        if mask >> d & 1:
            m = int(box[d] / rc)
            ci, cj = c[rows, d], c[cols, d]
            w = np.where((ci == 0) & (cj == m - 1), -1, np.where((ci == m - 1) & (cj == 0), 1, 0))
            pj[:, d] = pj[:, d] + (w.astype(T) * T(box[d]))
    dd = pj - p[rows]
    return (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]


def type_filter(kp, lst, q, rc, box, mask, dtype, types, rcm):
    """The canonical CSR (kp, lst) of the plain build filtered by the type table: (counts, kp, lst)."""
    kp = np.asarray(kp, dtype=np.int64)
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    cols = np.asarray(lst, dtype=np.int64)
    r2 = entry_r2(q, rc, box, mask, dtype, rows, cols)
    thr = rc2_table(rcm, dtype)
    t = np.asarray(types, dtype=np.int64)
    keep = ~(r2 > thr[t[rows], t[cols]])
    counts = np.bincount(rows[keep], minlength=n).astype(np.int32)
    kp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=kp2[1:])
    return counts, kp2, np.asarray(lst)[keep].astype(np.int32)


def seeded_types(n, ntypes, seed, rc=RC, zero=False):
    """Types (80:20-ish for 2) and a symmetric cut-off matrix in [0.6 rc, rc] with one rc_ab == rc (and one 0)."""
    rng = np.random.default_rng(seed)
    p = np.linspace(2.0, 1.0, ntypes)
    types = rng.choice(ntypes, size=n, p=p / p.sum()).astype(np.int32)
    a = rng.uniform(0.6 * rc, rc, size=(ntypes, ntypes))
    rcm = np.triu(a) + np.triu(a, 1).T
    rcm[0, 0] = rc
    if zero and ntypes > 1:
        rcm[-1, -1] = 0.0
    return types, rcm


# ------------------------------------------------------------------------------------------------------------- CPU
def brute_force(q, rc, box, mask, types, rcm, tol):
    """O(N^2) float64: per-axis minimum image on the axes of the mask; (pairs i < j kept, pairs within tol of their cut-off)."""
    p = q[:, :3].astype(np.float64)
    L = np.array(box, dtype=np.float64)
    per = np.array([bool(mask >> d & 1) for d in range(3)])
    keep, edge = set(), set()
    for i in range(len(p) - 1):
        d = p[i + 1:] - p[i]
        d[:, per] -= L[per] * np.round(d[:, per] / L[per])
        r = np.sqrt((d * d).sum(axis=1))
        js = np.arange(i + 1, len(p))
        cut = np.minimum(rcm[types[i], types[i + 1:]], rc)
        keep.update((i, int(j)) for j in js[r <= cut])
        edge.update((i, int(j)) for j in js[(np.abs(r - cut) <= tol * rc) | (np.abs(r - rc) <= tol * rc)])
    return keep, edge


@pytest.mark.parametrize("mask", range(8))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_type_filter_against_a_brute_force(mask, dtype):
    for seed, box, rc, n, nt in ((1, (12.0, 11.0, 14.0), 3.0, 1500, 2), (2, (10.5, 16.0, 9.9), 3.2, 1800, 3)):
        q = positions(n, box, rc, mask, dtype, seed + 10 * mask)
        types, rcm = seeded_types(n, nt, seed + mask, rc)
        rcm[-1, 0] = rcm[0, -1] = 0.5 * rc
        kp, lst = ref_list(q, rc, box, mask)
        _, kp2, lst2 = type_filter(kp, lst, q, rc, box, mask, dtype, types, rcm)
        rows = np.repeat(np.arange(n), np.diff(kp2))
        got = set(zip(rows.tolist(), lst2.tolist()))
        want, edge = brute_force(q, rc, box, mask, types, rcm, 1e-5 if dtype == np.float32 else 1e-12)
        assert got - edge == want - edge, (mask, seed, len(got ^ want))
        assert len(want) > 1000 and len(lst2) < len(lst)
        # full list: the same pairs in both rows
        fk, fl = ref_list(q, rc, box, mask, True)
        _, fk2, fl2 = type_filter(fk, fl, q, rc, box, mask, dtype, types, rcm)
        frows = np.repeat(np.arange(n), np.diff(fk2))
        fset = set(zip(frows.tolist(), fl2.tolist()))
        assert {(min(a, b), max(a, b)) for a, b in fset} - edge == want - edge


@pytest.mark.parametrize("name", golden_names(dup=True))
def test_type_filter_keeps_coincident_pairs(name):
    """The dup_* goldens (coincident particles; meshes below 3 cells, which the library refuses): rc_ab = 0 keeps exactly
    the pairs at distance 0, rc_ab = rc the whole list."""
    g = load_golden(name)
    q, rc, box = g["q"], float(g["rc"]), tuple(g["box"])
    dtype = q.dtype.type
    n = len(q)
    qq = np.concatenate([q, q[:3]])  # duplicates of three particles: distance 0
    kp, lst = _po_brute(qq, rc, dtype)
    types = np.zeros(len(qq), dtype=np.int32)
    _, kp0, lst0 = type_filter(kp, lst, qq, rc, (1e9, 1e9, 1e9), 0, dtype, types, [[0.0]])
    rows = np.repeat(np.arange(len(qq)), np.diff(kp0))
    assert set(zip(rows.tolist(), lst0.tolist())) == {(i, n + i) for i in range(3)}
    _, kp1, lst1 = type_filter(kp, lst, qq, rc, (1e9, 1e9, 1e9), 0, dtype, types, [[rc]])
    assert np.array_equal(kp1, kp) and np.array_equal(lst1, lst)


def _po_brute(q, rc, dtype):
    """Half list i < j with !(r2 > rc2) in dtype (no cells): (kp, lst)."""
    p = q[:, :3].astype(dtype)
    thr = floor_to(rc * rc, dtype)
    rows, cols = [], []
    for i in range(len(p) - 1):
        d = p[i + 1:] - p[i]
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        js = np.nonzero(~(r2 > thr))[0] + i + 1
        rows += [i] * len(js)
        cols += js.tolist()
    kp = np.zeros(len(p) + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.array(rows, dtype=np.int64), minlength=len(p)), out=kp[1:])
    return kp, np.array(cols, dtype=np.int32)


def test_exports():
    from md_neighbor_list_amd import _lib

    names = ("nl_set_type_cutoffs", "nl_get_types", "nl_set_lj_type_params", "nl_lj_forces_typed", "nl_lj_forces_typed_enqueue")
    lib = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "nl_hip.h")) as f:
        hdr = f.read()
    assert "#define NL_MAX_TYPES 32" in hdr and _lib.NL_MAX_TYPES == 32
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and f"int {name}(" in hdr, name


# ------------------------------------------------------------------------------------------------------------- GPU
def _handle(n, dtype, mask=0, full=False, rc=RC, box=BOX):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full)
    if mask:
        nl.set_periodic(axes=tuple(bool(mask >> d & 1) for d in range(3)))
    nl.Initialize(n)
    return nl


def _list(nl):
    if nl.full_list:
        kp, lst, cnt = (t.cpu().numpy() for t in nl.full_csr())
    else:
        kp, lst, cnt = (t.cpu().numpy() for t in (nl.key_pointer(), nl.sorted_list(), nl.half_number_of_partners()))
    return kp.astype(np.int64), lst, cnt


def _build(nl, q, sync=True):
    torch = _torch()
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(qd, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return qd


def _assert_list(nl, want, what=""):
    counts, kp_w, lst_w = want
    kp, lst, cnt = _list(nl)
    assert np.array_equal(cnt, counts), what
    assert np.array_equal(kp, kp_w), what
    assert np.array_equal(canonical_csr(kp, lst), lst_w), what
    assert nl.half_number_of_pairs() == (len(lst_w) // 2 if nl.full_list else len(lst_w)), what


def _want(q, rc, box, mask, full, dtype, types, rcm, pairs=None):
    kp, lst = ref_list(q, rc, box, mask, full)
    w = type_filter(kp, lst, q, rc, box, mask, dtype, types, rcm)
    if pairs is not None:
        w = remove_pairs(w[1], w[2], pairs)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", [g for g in golden_names(dup=False) if g.endswith("_f32")])
def test_goldens(name, dtype):
    g = load_golden(name)
    q, rc, box = g["q"].astype(dtype), float(g["rc"]), tuple(g["box"])
    n = len(q)
    for ci, nt in enumerate((1, 2, 3, 5)):
        types, rcm = seeded_types(n, nt, 7 + ci, rc, zero=True)
        if nt == 1:
            rcm[0, 0] = 0.8 * rc
        for full in (False, True):
            nl = _handle(n, dtype, 0, full, rc, box)
            nl.set_type_cutoffs(types, rcm)
            _build(nl, q)
            _assert_list(nl, _want(q, rc, box, 0, full, dtype, types, rcm), (name, nt, full))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_all_masks(dtype):
    """All rc_ab == rc: the plain list (canonical CSR and checksum), every mask, half and full."""
    n = 12000
    for mask in range(8):
        q = positions(n, BOX, RC, mask, dtype, 200 + mask)
        types, _ = seeded_types(n, 3, 300 + mask)
        for full in (False, True):
            nl = _handle(n, dtype, mask, full)
            _build(nl, q)
            kp0, lst0, cnt0 = (a.copy() for a in _list(nl))
            cs0 = nl.list_checksum()
            nl.set_type_cutoffs(types, np.full((3, 3), RC))
            _build(nl, q)
            kp1, lst1, cnt1 = _list(nl)
            assert np.array_equal(kp0, kp1) and np.array_equal(cnt0, cnt1), (mask, full)
            assert np.array_equal(canonical_csr(kp0, lst0), canonical_csr(kp1, lst1)), (mask, full)
            assert nl.list_checksum() == cs0
            # and a real table on the same handle
            types2, rcm = seeded_types(n, 3, 400 + mask, zero=True)
            nl.set_type_cutoffs(types2, rcm)
            _build(nl, q)
            _assert_list(nl, _want(q, RC, BOX, mask, full, dtype, types2, rcm), (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("env", [("NL_SWEEP_VARIANT", "1"), ("NL_SWEEP_VARIANT", "3"), ("NL_ROWS", "0"), ("NL_ROWS", "4"),
                                 ("NL_BINNING", "1"), ("NL_OFFSET_WIDTH", "64")])
def test_search_paths(env, monkeypatch):
    monkeypatch.setenv(*env)
    if env[0] == "NL_ROWS":
        q, box = inputs.uniform_box(40000, dtype=np.float32, seed=5, box=(33.0, 33.0, 33.9))
    else:
        q, box = positions(20000, BOX, RC, 0, np.float32, 50), BOX
    n = len(q)
    types, rcm = seeded_types(n, 2, 51)
    for full in (False, True):
        nl = _handle(n, np.float32, 0, full, RC, box)
        _build(nl, q)
        kp0, lst0, _ = (a.copy() for a in _list(nl))
        cs0 = nl.list_checksum()
        nl.set_type_cutoffs(types, np.full((2, 2), RC))
        _build(nl, q)
        kp1, lst1, _ = _list(nl)
        assert np.array_equal(kp0, kp1) and np.array_equal(canonical_csr(kp0, lst0), canonical_csr(kp1, lst1))
        assert nl.list_checksum() == cs0
        info = nl.build_info()
        if env == ("NL_ROWS", "4"):
            assert info["fine_rows"] > 0, info
        if env == ("NL_OFFSET_WIDTH", "64"):
            assert info["offset_bits"] == 64
        nl.set_type_cutoffs(types, rcm)
        _build(nl, q)
        _assert_list(nl, _want(q, RC, box, 0, full, np.float32, types, rcm), (env, full))


def _band_case(dtype, mask, seed):
    """Pairs at rc_ab (1 + k ulp), k = -3 .. 3, of every type pair, inside the box and across the periodic faces."""
    rng = np.random.default_rng(seed)
    box = (40.0, 40.0, 40.0)
    rcm = np.array([[3.3, 2.64], [2.64, 2.904]])
    pts, types = [], []
    slot = 0
    for a in range(2):
        for b in range(2):
            r = dtype(rcm[a, b])
            for k in range(-3, 4):
                d = r
                for _ in range(abs(k)):
                    d = np.nextafter(d, dtype(np.inf) if k > 0 else dtype(0))
                for axis in range(3):
                    for across in (False, True):
                        # anchors on a coarse lattice (other pairs between them are decided by the same rule)
                        base = np.array([4.0 + 6.0 * (slot % 6), 4.0 + 6.0 * ((slot // 6) % 6), 4.0 + 6.0 * (slot // 36)])
                        slot += 1
                        p0 = base.copy()
                        p1 = base.copy()
                        if across:
                            p0[axis] = float(rng.uniform(0.0, 0.5))
                            p1[axis] = float(dtype(p0[axis]) - d) + box[axis]
                        else:
                            p1[axis] = float(dtype(p0[axis]) + d)
                        pts += [p0, p1]
                        types += [a, b]
    q = np.zeros((len(pts), 4), dtype=dtype)
    q[:, :3] = np.array(pts).astype(dtype)
    return q, box, np.array(types, dtype=np.int32), rcm


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cutoff_band(dtype):
    for mask in (0, 7):
        q, box, types, rcm = _band_case(dtype, mask, 60)
        n = len(q)
        for full in (False, True):
            want = _want(q, RC, box, mask, full, dtype, types, rcm)
            plain = ref_list(q, RC, box, mask, full)
            assert 0 < len(want[2]) < len(plain[1])  # the band decides both ways
            nl = _handle(n, dtype, mask, full, RC, box)
            nl.set_type_cutoffs(types, rcm)
            _build(nl, q)
            _assert_list(nl, want, (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_types_and_exclusions(dtype):
    n = 20000
    for mask in (0, 5):
        q = positions(n, BOX, RC, mask, dtype, 70 + mask)
        types, rcm = seeded_types(n, 3, 71)
        for full in (False, True):
            kp, lst = ref_list(q, RC, BOX, mask, full)
            pairs = mixed_pairs(kp, lst, n, 72)
            nl = _handle(n, dtype, mask, full)
            nl.set_exclusions(pairs, n)
            nl.set_type_cutoffs(types, rcm)
            _build(nl, q)
            _assert_list(nl, _want(q, RC, BOX, mask, full, dtype, types, rcm, pairs), (mask, full))
            nl.clear_exclusions()  # the type table alone again
            _build(nl, q)
            _assert_list(nl, _want(q, RC, BOX, mask, full, dtype, types, rcm), (mask, full))
            nl.set_exclusions(pairs, n)
            nl.clear_type_cutoffs()  # the exclusions alone
            _build(nl, q)
            _assert_list(nl, remove_pairs(kp, lst, pairs), (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_checksum_transposed_and_pairs(full):
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 80)
    types, rcm = seeded_types(n, 2, 81)
    _, kp_w, lst_w = _want(q, RC, BOX, 0, full, np.float32, types, rcm)
    nl = _handle(n, np.float32, 0, full)
    nl.set_type_cutoffs(types, rcm)
    _build(nl, q)
    cs, ne = nl.list_checksum()
    assert ne == len(lst_w) and cs == _checksum(kp_w, lst_w)
    npairs = C.c_int64()
    assert nl._lib.nl_number_of_pairs(nl._h, C.byref(npairs)) == 0
    assert npairs.value == (len(lst_w) // 2 if full else len(lst_w))
    assert nl.number_of_pairs() == 2 * npairs.value
    fk, fl = (kp_w, lst_w) if full else full_from_half(kp_w, lst_w)
    t = nl.neigh_list().cpu().numpy()
    cnt = nl.number_of_partners().cpu().numpy()
    assert np.array_equal(cnt[:n], np.diff(fk))
    got = np.concatenate([np.sort(t[:cnt[i], i]) for i in range(n)])
    assert np.array_equal(got, fl)


@pytest.mark.gpu
def test_growth_and_capacity():
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 90)
    types, _ = seeded_types(n, 2, 91)
    rcm = np.array([[2.0, 1.5], [1.5, 1.0]])
    for full in (False, True):
        plain = ref_list(q, RC, BOX, 0, full)
        want = _want(q, RC, BOX, 0, full, np.float32, types, rcm)
        nl = _handle(n, np.float32, 0, full)
        nl.set_type_cutoffs(types, rcm)
        nl.set_capacity(len(plain[1]) // 3)
        _build(nl, q)
        _assert_list(nl, want, full)
        nl2 = _handle(n, np.float32, 0, full)
        nl2.set_type_cutoffs(types, rcm)
        cap = (len(want[2]) + len(plain[1])) // 2
        assert len(want[2]) < cap < len(plain[1])
        nl2.set_capacity(cap)
        with pytest.raises(NLError) as e:
            _build(nl2, q, sync=False)
        assert e.value.code == NL_ERR_CAPACITY


@pytest.mark.gpu
def test_graph_replay_and_update():
    torch = _torch()
    n = 8000
    box = (20.0, 20.0, 20.0)
    q = positions(n, box, RC, 0, np.float32, 100)
    types, rcm = seeded_types(n, 2, 101)
    nl = _handle(n, np.float32, 0, False, RC, box)
    nl.set_graph(True)
    nl.set_type_cutoffs(types, rcm)
    qd = torch.from_numpy(q).cuda()
    for step in range(2):
        nl.MakeNeighList(qd, n, sync=False)
        nl.synchronize()
        _assert_list(nl, _want(q, RC, box, 0, False, np.float32, types, rcm), step)
    rcm2 = rcm * 0.9  # a new table is a new graph
    nl.set_type_cutoffs(types, rcm2)
    nl.MakeNeighList(qd, n, sync=False)
    nl.synchronize()
    _assert_list(nl, _want(q, RC, box, 0, False, np.float32, types, rcm2))
    # nl_update_list: skipped updates keep the list, a new table forces a build
    nl2 = _handle(n, np.float32, 0, False, RC, box)
    nl2.set_skin(0.3)
    nl2.update(qd, sync=True)
    _, b0 = nl2.update_stats()
    nl2.set_type_cutoffs(types, rcm)
    nl2.update(qd, sync=True)
    assert nl2.update_stats()[1] == b0 + 1
    nl2.update(qd, sync=True)
    assert nl2.update_stats()[1] == b0 + 1
    _assert_list(nl2, _want(q, RC, box, 0, False, np.float32, types, rcm))
    nl2.set_type_cutoffs(types, rcm2)
    nl2.update(qd, sync=True)
    assert nl2.update_stats()[1] == b0 + 2
    _assert_list(nl2, _want(q, RC, box, 0, False, np.float32, types, rcm2))


@pytest.mark.gpu
def test_resort_relabels_the_types():
    torch = _torch()
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 120)
    types, rcm = seeded_types(n, 3, 121)
    nl = _handle(n, np.float32)
    nl.set_type_cutoffs(types, rcm)
    qd = _build(nl, q)
    order = nl.cell_order().cpu().numpy().copy()
    ptr = nl.types().data_ptr()
    vel = torch.arange(n, dtype=torch.int32, device="cuda")
    nl.resort(qd, vel)  # (two arrays: the types are relabelled once)
    torch.cuda.synchronize()
    assert np.array_equal(vel.cpu().numpy(), order)
    assert nl.types().data_ptr() == ptr
    assert np.array_equal(nl.types().cpu().numpy(), types[order])
    nl.MakeNeighList(qd, n)
    _assert_list(nl, _want(q[order], RC, BOX, 0, False, np.float32, types[order], rcm))


@pytest.mark.gpu
def test_captured_step_survives_a_resort():
    torch = _torch()
    n = 8000
    box = (20.0, 20.0, 20.0)
    rng = np.random.default_rng(150)
    g = np.stack(np.meshgrid(*(np.arange(20),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = np.zeros((n, 4), dtype=np.float32)
    q[:, :3] = 0.5 + 0.9 * g + rng.uniform(-0.05, 0.05, size=(n, 3))
    q = q[rng.permutation(n)]
    types, rcm = seeded_types(n, 2, 151)
    nl = _handle(n, np.float32, 0, False, RC, box)
    nl.set_skin(0.3)
    nl.set_type_cutoffs(types, rcm)
    nl.set_lj_type_params(np.ones((2, 2)), np.full((2, 2), 0.8), rcm - 0.3)
    qd = torch.from_numpy(q).cuda()
    f = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    nl.update(qd, sync=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nl.update(qd)
        nl.lj_forces_typed(qd, wait=False, out=f)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=s):
        nl.update(qd)
        nl.lj_forces_typed(qd, wait=False, out=f)
    cg.replay()
    torch.cuda.synchronize()
    order = nl.cell_order().cpu().numpy().copy()
    nl.resort(qd)
    nl.update(qd, sync=True)  # (forced: the re-sort)
    qp, tp = q[order].copy(), types[order]
    for step in range(2):
        qp[:, :3] += rng.uniform(-0.1, 0.1, size=(n, 3)).astype(np.float32) + np.float32(0.2)
        qd.copy_(torch.from_numpy(qp))
        b0 = nl.update_stats()[1]
        cg.replay()
        torch.cuda.synchronize()
        assert nl.update_stats()[1] == b0 + 1
        _assert_list(nl, _want(qp, RC, box, 0, False, np.float32, tp, rcm), step)
        assert torch.isfinite(f).all()


@pytest.mark.gpu
def test_errors_keep_the_old_table():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    torch = _torch()
    n = 4000
    box = (20.0, 20.0, 20.0)
    q = positions(n, box, RC, 0, np.float32, 140)
    nl = _handle(n, np.float32, 0, False, RC, box)
    with pytest.raises(NLError) as e:
        nl.types()
    assert e.value.code == NL_ERR_STATE
    types, rcm = seeded_types(n, 2, 141)
    nl.set_type_cutoffs(types, rcm)
    bad_types = types.copy()
    bad_types[17] = 2
    neg = types.copy()
    neg[5] = -1
    asym = rcm.copy()
    asym[0, 1] = np.nextafter(asym[0, 1], 0.0)
    nan = rcm.copy()
    nan[1, 1] = np.nan
    big = rcm.copy()
    big[0, 0] = np.nextafter(RC, 10.0)
    cases = [(bad_types, rcm), (neg, rcm), (types, asym), (types, nan), (types, big),
             (np.zeros(n, dtype=np.int32), np.full((33, 33), 1.0)), (np.zeros(n + 1, dtype=np.int32), rcm)]
    for t, m in cases:
        with pytest.raises(NLError) as e:
            nl.set_type_cutoffs(t, m)
        assert e.value.code == NL_ERR_ARG
        assert np.array_equal(nl.types().cpu().numpy(), types)  # the old table is kept
    qd = torch.from_numpy(q).cuda()
    with pytest.raises(NLError) as e:  # a build of another particle count
        nl.MakeNeighList(qd, n - 1)
    assert e.value.code == NL_ERR_ARG
    with pytest.raises(NLError) as e:  # slab builds are out of scope
        nl.MakeNeighListSlab(qd, torch.arange(n, dtype=torch.int32, device="cuda"), n, 0, nl.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    with pytest.raises(NLError) as e:
        nl.MakeNeighListSlabBegin(qd, None, n, 0, 0, nl.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    from md_neighbor_list_amd._lib import load

    lib = load()
    # (refused before the communicator is looked at: a table is checked first)
    assert lib.nl_make_list_distributed(nl._h, C.c_void_p(1), qd.data_ptr(), n, n, None, 1) == NL_ERR_STATE
    nl.MakeNeighList(qd, n)
    _assert_list(nl, _want(q, RC, box, 0, False, np.float32, types, rcm))
    nl.clear_type_cutoffs()
    with pytest.raises(NLError):
        nl.types()


def _lj_ref(q, kp, lst, types, eps, sig, rcf, box, mask, with_bound=False):
    n = len(q)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    cols = np.asarray(lst, dtype=np.int64)
    ti, tj = types[rows], types[cols]
    d = lj_list_separations(q, rows, cols, (*box, 0.0, 0.0, 0.0), mask)  # (folded before it is rounded to float64)
    r2 = (d * d).sum(axis=1)
    inr = r2 < rcf[ti, tj] ** 2
    s2 = sig[ti, tj] ** 2 / r2
    s6 = s2 ** 3
    fr = np.where(inr, 24.0 * eps[ti, tj] * (2.0 * s6 * s6 - s6) / r2, 0.0)
    pe = np.where(inr, 4.0 * eps[ti, tj] * (s6 * s6 - s6), 0.0)
    out = np.zeros((n, 4))
    for c in range(3):
        np.add.at(out[:, c], rows, fr * d[:, c])
        np.add.at(out[:, c], cols, -fr * d[:, c])
    np.add.at(out[:, 3], rows, 0.5 * pe)
    np.add.at(out[:, 3], cols, 0.5 * pe)
    if with_bound:  # (S of check_lj, and the particles off the 64-ulp band of their pairs' rc_force)
        S = lj_pair_magnitudes(n, rows, cols, d, r2, eps[ti, tj], sig[ti, tj], inr)
        return out, S, lj_rows_off_the_band(n, rows, cols, r2, rcf[ti, tj], q.dtype)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("mask", [0, 3])
def test_lj_forces_typed(dtype, full, mask):
    torch = _torch()
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    rc, box = 3.0, (30.0, 30.0, 30.0)
    rng = np.random.default_rng(160)
    g = np.stack(np.meshgrid(*(np.arange(25),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = np.zeros((len(g), 4), dtype=dtype)
    q[:, :3] = (0.6 + 1.2 * g + rng.uniform(-0.1, 0.1, size=g.shape)).astype(dtype)  # no pair closer than 1.0
    n = len(q)
    types = (rng.uniform(size=n) < 0.2).astype(np.int32)
    rcm = np.array([[2.8, 2.64], [2.64, 2.904]])
    eps = np.array([[1.0, 1.5], [1.5, 0.5]])
    sig = np.array([[1.0, 0.8], [0.8, 0.88]])
    rcf = 2.5 * sig
    nl = _handle(n, dtype, mask, full, rc, box)
    with pytest.raises(NLError) as e:
        nl.set_lj_type_params(eps, sig, rcf)  # no type table
    assert e.value.code == NL_ERR_STATE
    nl.set_type_cutoffs(types, rcm)
    qd = _build(nl, q)
    with pytest.raises(NLError) as e:
        nl.lj_forces_typed(qd)  # no parameters
    assert e.value.code == NL_ERR_STATE
    with pytest.raises(NLError) as e:
        nl.set_lj_type_params(eps, sig, rcm + 0.01)  # rc_force beyond rc_ab
    assert e.value.code == NL_ERR_ARG
    with pytest.raises(NLError) as e:
        nl.set_lj_type_params(np.ones((3, 3)), np.ones((3, 3)), np.ones((3, 3)))  # another ntypes
    assert e.value.code == NL_ERR_ARG
    nl.set_lj_type_params(eps, sig, rcf)
    got = nl.lj_forces_typed(qd).cpu().numpy().astype(np.float64)
    _, kp_w, lst_w = _want(q, rc, box, mask, False, dtype, types, rcm)
    want, S, off_band = _lj_ref(q, kp_w, lst_w, types, eps, sig, rcf, box, mask, with_bound=True)
    scale = np.abs(want).max(axis=0)
    tol = 2e-4 if dtype == np.float32 else 1e-11
    assert np.all(np.abs(got - want) <= tol * scale), (np.abs(got - want) / scale).max(axis=0)
    check_lj(got, want, S, dtype, rows=off_band)  # per particle and component within c u S (tests/test_lj_consumer.py)
    # the enqueue variant: rc_force within rc_ab - skin
    nl.set_skin(0.5)
    nl.update(qd, sync=True)
    with pytest.raises(NLError) as e:
        nl.lj_forces_typed(qd, wait=False)  # rc_force_AA = 2.5 > rc_AA - skin = 2.3
    assert e.value.code == NL_ERR_ARG
    nl.set_lj_type_params(eps, sig, np.minimum(rcf, rcm - 0.5))
    f = nl.lj_forces_typed(qd, wait=False)
    torch.cuda.synchronize()
    want2, S2, off_band2 = _lj_ref(q, kp_w, lst_w, types, eps, sig, np.minimum(rcf, rcm - 0.5), box, mask, with_bound=True)
    assert np.all(np.abs(f.cpu().numpy().astype(np.float64) - want2) <= tol * np.abs(want2).max(axis=0))
    check_lj(f.cpu().numpy(), want2, S2, dtype, rows=off_band2)

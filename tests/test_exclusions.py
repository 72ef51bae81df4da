"""Excluded pairs (nl_set_exclusions): a build with a table lists exactly the pairs of the plain build minus the pairs of the
table, in either order.

The reference is the oracle's list -- pyoracle.build for the open box (the full list mirrored from the half one), and the
padded-box construction of tests/test_periodic_axes.py for periodic masks -- with the excluded pairs removed in numpy
(`remove_pairs`, itself checked against a brute force on the CPU).  Every GPU list is compared after the reference's
canonical sort, bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.test_periodic_axes import positions, reference
from tests.util import ROOT, canonical_csr, check_lj, lj_pair_magnitudes, lj_rows_off_the_band, load_golden

BOX = (27.0, 24.0, 40.0)
RC = 3.3


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


# ------------------------------------------------------------------------------------------------- numpy reference
def remove_pairs(kp, lst, pairs):
    """The canonical CSR (kp, lst) without the pairs {i, j} of `pairs` in either order: (counts, kp, lst)."""
    kp = np.asarray(kp, dtype=np.int64)
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    key = (rows << 32) | np.asarray(lst, dtype=np.int64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ex = np.concatenate([(p[:, 0] << 32) | p[:, 1], (p[:, 1] << 32) | p[:, 0]])
    keep = ~np.isin(key, ex)
    counts = np.bincount(rows[keep], minlength=n).astype(np.int32)
    kp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=kp2[1:])
    return counts, kp2, np.asarray(lst)[keep].astype(np.int32)


def table_csr(pairs, n):
    """The table nl_get_exclusions returns: symmetric, per-row ascending, without duplicates."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    key = np.unique(np.concatenate([(p[:, 0] << 32) | p[:, 1], (p[:, 1] << 32) | p[:, 0]]))
    rows = key >> 32
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    return off, (key & 0xFFFFFFFF).astype(np.int32)


def full_from_half(kp, lst):
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    cols = np.asarray(lst, dtype=np.int64)
    a, b = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    key = (a << 32) | b
    key.sort()
    counts = np.bincount(key >> 32, minlength=n)
    kp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=kp2[1:])
    return kp2, (key & 0xFFFFFFFF).astype(np.int32)


def ref_list(q, rc, box, mask=0, full=False):
    """(kp, lst) of the plain build, canonical."""
    if mask == 0 and (q[:, :3] >= 0).all() and (q[:, :3] < np.asarray(box)).all():
        h = _po().build(q, rc, box).canonical()
        return full_from_half(h.key_pointer, h.sorted_list) if full else (h.key_pointer, h.sorted_list)
    r = reference(q, rc, box, mask, full)
    return r.key_pointer, r.sorted_list


def mixed_pairs(kp, lst, n, seed, k=None):
    """Pairs within the cut-off (taken from the list), pairs beyond it, duplicates and both orders."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    k = k or max(len(lst) // 10, 16)
    pick = rng.choice(len(lst), size=min(k, len(lst)), replace=False)
    near = np.stack([rows[pick], np.asarray(lst)[pick].astype(np.int64)], axis=1)
    far = rng.integers(0, n, size=(k, 2))
    far = far[far[:, 0] != far[:, 1]]
    dup = near[: len(near) // 4]
    rev = near[len(near) // 4: len(near) // 2][:, ::-1]
    out = np.concatenate([near, far, dup, rev])
    return out[rng.permutation(len(out))].astype(np.int32)


def test_remove_pairs_against_a_brute_force():
    """CPU: remove_pairs on the oracle's list equals an O(N^2) set-based list minus the excluded set."""
    for seed, (n, L) in enumerate(((300, 10.0), (600, 11.5))):
        rng = np.random.default_rng(seed)
        q = np.zeros((n, 4), dtype=np.float64)
        q[:, :3] = rng.uniform(0.0, L, size=(n, 3))
        box = (L, L, L)
        rc = 3.0
        kp, lst = ref_list(q, rc, box)
        pairs = mixed_pairs(kp, lst, n, seed)
        _, kp2, lst2 = remove_pairs(kp, lst, pairs)
        ex = {(int(a), int(b)) for a, b in pairs} | {(int(b), int(a)) for a, b in pairs}
        want = set()
        p = q[:, :3]
        for i in range(n - 1):
            d = p[i + 1:] - p[i]
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            for j in np.nonzero(r2 <= rc * rc)[0] + i + 1:
                if (i, int(j)) not in ex:
                    want.add((i, int(j)))
        rows = np.repeat(np.arange(n), np.diff(kp2))
        assert set(zip(rows.tolist(), lst2.tolist())) == want
        assert len(lst2) == len(want)
        # and the table: symmetric, deduplicated
        off, ids = table_csr(pairs, n)
        trow = np.repeat(np.arange(n), np.diff(off))
        assert set(zip(trow.tolist(), ids.tolist())) == ex


def test_exports():
    """The built library exports the two entry points and _lib declares them."""
    from md_neighbor_list_amd import _lib

    for name in ("nl_set_exclusions", "nl_get_exclusions"):
        assert name in _lib.PROTOTYPES
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("nl_set_exclusions", "nl_get_exclusions"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "nl_hip.h")) as f:
        hdr = f.read()
    assert "int nl_set_exclusions(" in hdr and "int nl_get_exclusions(" in hdr


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


def _assert_filtered(nl, kp_ref, lst_ref, pairs, what=""):
    counts, kp_w, lst_w = remove_pairs(kp_ref, lst_ref, pairs)
    kp, lst, cnt = _list(nl)
    assert np.array_equal(cnt, counts), what
    assert np.array_equal(kp, kp_w), what
    assert np.array_equal(canonical_csr(kp, lst), lst_w), what
    npairs = nl.half_number_of_pairs()
    assert npairs == (len(lst_w) // 2 if nl.full_list else len(lst_w)), what
    return kp, lst


def _build(nl, q, sync=True):
    torch = _torch()
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(qd, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return qd


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_half_and_full_lists(dtype):
    g = load_golden("u4096_rho1_f32")
    cases = [(positions(20000, BOX, RC, 0, dtype, 11), RC, BOX), (g["q"].astype(dtype), float(g["rc"]), tuple(g["box"]))]
    for ci, (q, rc, box) in enumerate(cases):
        n = len(q)
        for full in (False, True):
            kp_ref, lst_ref = ref_list(q, rc, box, 0, full)
            pairs = mixed_pairs(kp_ref, lst_ref, n, 20 + ci)
            nl = _handle(n, dtype, 0, full, rc, box)
            nl.set_exclusions(pairs, n)
            _build(nl, q)
            _assert_filtered(nl, kp_ref, lst_ref, pairs, (ci, full))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hub_and_a_whole_row(dtype):
    """A hub with >= 200 exclusions (binary search in its sorted segment) and a row excluded entirely."""
    q = positions(20000, BOX, RC, 0, dtype, 12)
    n = len(q)
    rng = np.random.default_rng(3)
    for full in (False, True):
        kp_ref, lst_ref = ref_list(q, RC, BOX, 0, full)
        hub, whole = 17, 4242
        own = lst_ref[kp_ref[hub]:kp_ref[hub + 1]].astype(np.int64)
        others = rng.choice(np.setdiff1d(np.arange(n), [hub]), 240, replace=False)
        hub_pairs = np.stack([np.full(len(own) + 240, hub), np.concatenate([own, others])], axis=1)
        row = lst_ref[kp_ref[whole]:kp_ref[whole + 1]].astype(np.int64)
        assert len(row) > 0
        row_pairs = np.stack([row, np.full(len(row), whole)], axis=1)  # (the other order)
        pairs = np.concatenate([hub_pairs, row_pairs]).astype(np.int32)
        nl = _handle(n, dtype, 0, full)
        nl.set_exclusions(pairs, n)
        _build(nl, q)
        kp, lst, cnt = _list(nl)
        _assert_filtered(nl, kp_ref, lst_ref, pairs, full)
        assert cnt[whole] == 0
        off, _ = (t.cpu().numpy() for t in nl.exclusions())
        assert off[hub + 1] - off[hub] >= 200


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_masks(dtype):
    n = 20000
    for mask in (0, 3, 7):
        q = positions(n, BOX, RC, mask, dtype, 30 + mask)
        for full in (False, True):
            kp_ref, lst_ref = ref_list(q, RC, BOX, mask, full)
            pairs = mixed_pairs(kp_ref, lst_ref, n, 40 + mask)
            nl = _handle(n, dtype, mask, full)
            nl.set_exclusions(pairs, n)
            _build(nl, q)
            _assert_filtered(nl, kp_ref, lst_ref, pairs, (mask, full))


@pytest.mark.gpu
@pytest.mark.parametrize("env", [("NL_SWEEP_VARIANT", "1"), ("NL_SWEEP_VARIANT", "3"), ("NL_ROWS", "0"), ("NL_ROWS", "4"),
                                 ("NL_BINNING", "1"), ("NL_OFFSET_WIDTH", "64")])
def test_search_paths(env, monkeypatch):
    monkeypatch.setenv(*env)
    if env[0] == "NL_ROWS":  # a box the fine-row search takes under NL_ROWS=4 (tests/test_gpu_parity.py)
        q, box = inputs.uniform_box(40000, dtype=np.float32, seed=5, box=(33.0, 33.0, 33.9))
    else:
        q, box = positions(20000, BOX, RC, 0, np.float32, 50), BOX
    n = len(q)
    for full in (False, True):
        kp_ref, lst_ref = ref_list(q, RC, box, 0, full)
        pairs = mixed_pairs(kp_ref, lst_ref, n, 51)
        nl = _handle(n, np.float32, 0, full, RC, box)
        nl.set_exclusions(pairs, n)
        _build(nl, q)
        info = nl.build_info()
        if env[0] == "NL_SWEEP_VARIANT":
            assert info["variant"] == int(env[1]) and info["masks"] == (env[1] == "3"), info
        if env == ("NL_ROWS", "4"):
            assert info["fine_rows"] > 0, info
        if env == ("NL_ROWS", "0"):
            assert info["fine_rows"] == 0, info
        if env == ("NL_OFFSET_WIDTH", "64"):
            assert info["offset_bits"] == 64
            kp64 = (nl.full_csr(64)[0] if full else nl.key_pointer64()).cpu().numpy()
            assert np.array_equal(kp64, remove_pairs(kp_ref, lst_ref, pairs)[1])
        _assert_filtered(nl, kp_ref, lst_ref, pairs, (env, full))


@pytest.mark.gpu
def test_dense_fp64_box():
    n = 60000
    q = positions(n, BOX, RC, 3, np.float64, 60)
    for full in (False, True):
        kp_ref, lst_ref = ref_list(q, RC, BOX, 3, full)
        pairs = mixed_pairs(kp_ref, lst_ref, n, 61)
        nl = _handle(n, np.float64, 3, full)
        nl.set_exclusions(pairs, n)
        _build(nl, q)
        assert nl.build_info()["mask_rows"] > 1
        _assert_filtered(nl, kp_ref, lst_ref, pairs, full)


@pytest.mark.gpu
def test_table_and_clear():
    """nl_get_exclusions against numpy's symmetric, deduplicated CSR; clearing restores the plain list and checksum."""
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 70)
    kp_ref, lst_ref = ref_list(q, RC, BOX)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 71)
    nl = _handle(n, np.float32)
    _build(nl, q)
    kp0, lst0, cnt0 = (a.copy() for a in _list(nl))
    cs0 = nl.list_checksum()
    with pytest.raises(Exception):
        nl.exclusions()
    nl.set_exclusions(torch_pairs(pairs, np.int64), n)
    off, ids = (t.cpu().numpy() for t in nl.exclusions())
    off_w, ids_w = table_csr(pairs, n)
    assert np.array_equal(off, off_w) and np.array_equal(ids, ids_w)
    _build(nl, q)
    _assert_filtered(nl, kp_ref, lst_ref, pairs)
    assert nl.list_checksum() != cs0
    nl.clear_exclusions()
    with pytest.raises(Exception):
        nl.exclusions()
    _build(nl, q)
    kp1, lst1, cnt1 = _list(nl)
    assert np.array_equal(kp0, kp1) and np.array_equal(cnt0, cnt1)
    assert np.array_equal(canonical_csr(kp0, lst0), canonical_csr(kp1, lst1))
    assert nl.list_checksum() == cs0


def torch_pairs(pairs, dtype):
    torch = _torch()
    return torch.from_numpy(np.asarray(pairs, dtype=dtype)).cuda()


def _checksum(kp, lst):
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(kp))
    v = (rows << np.uint64(32)) | np.asarray(lst, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = v * np.uint64(0x9E3779B97F4A7C15)
        v ^= v >> np.uint64(29)
        return int(v.sum(dtype=np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_checksum_and_transposed(full):
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 80)
    kp_ref, lst_ref = ref_list(q, RC, BOX, 0, full)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 81)
    _, kp_w, lst_w = remove_pairs(kp_ref, lst_ref, pairs)
    nl = _handle(n, np.float32, 0, full)
    nl.set_exclusions(pairs, n)
    _build(nl, q)
    cs, ne = nl.list_checksum()
    assert ne == len(lst_w) and cs == _checksum(kp_w, lst_w)
    fk, fl = (kp_w, lst_w) if full else full_from_half(kp_w, lst_w)
    t = nl.neigh_list().cpu().numpy()
    cnt = nl.number_of_partners().cpu().numpy()
    assert np.array_equal(cnt[:n], np.diff(fk))
    got = np.concatenate([np.sort(t[:cnt[i], i]) for i in range(n)])
    assert np.array_equal(got, fl)


@pytest.mark.gpu
def test_growth_and_capacity():
    """A too-small capacity: the synchronous build grows and its re-run is filtered; an asynchronous build whose
    UNFILTERED list exceeds the capacity reports NL_ERR_CAPACITY even when the filtered one would fit."""
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 90)
    for full in (False, True):
        kp_ref, lst_ref = ref_list(q, RC, BOX, 0, full)
        pairs = mixed_pairs(kp_ref, lst_ref, n, 91, k=len(lst_ref) // 4)
        _, _, lst_w = remove_pairs(kp_ref, lst_ref, pairs)
        nl = _handle(n, np.float32, 0, full)
        nl.set_exclusions(pairs, n)
        nl.set_capacity(len(lst_ref) // 3)
        _build(nl, q)
        _assert_filtered(nl, kp_ref, lst_ref, pairs, full)
        nl2 = _handle(n, np.float32, 0, full)
        nl2.set_exclusions(pairs, n)
        cap = (len(lst_w) + len(lst_ref)) // 2
        assert len(lst_w) < cap < len(lst_ref)
        nl2.set_capacity(cap)
        with pytest.raises(NLError) as e:
            _build(nl2, q, sync=False)
        assert e.value.code == NL_ERR_CAPACITY


@pytest.mark.gpu
def test_graph_replay():
    torch = _torch()
    n = 8000
    box = (20.0, 20.0, 20.0)
    q0 = positions(n, box, RC, 0, np.float32, 100)
    kp_ref, lst_ref = ref_list(q0, RC, box)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 101)
    nl = _handle(n, np.float32, 0, False, RC, box)
    nl.set_graph(True)
    nl.set_exclusions(pairs, n)
    qd = torch.from_numpy(q0).cuda()
    rng = np.random.default_rng(102)
    for step in range(3):
        q = q0.copy()
        if step:
            q[:, :3] = np.clip(q[:, :3] + rng.normal(0, 0.05, size=(n, 3)).astype(np.float32), 0.0, 19.999)
        qd.copy_(torch.from_numpy(q))
        nl.MakeNeighList(qd, n, sync=False)
        nl.synchronize()
        kr, lr = ref_list(q, RC, box)
        _assert_filtered(nl, kr, lr, pairs, step)
    pairs2 = pairs[: len(pairs) // 2]  # a new table is a new graph
    nl.set_exclusions(pairs2, n)
    nl.MakeNeighList(qd, n, sync=False)
    nl.synchronize()
    _assert_filtered(nl, kr, lr, pairs2)


@pytest.mark.gpu
def test_skin_update_and_capture():
    torch = _torch()
    n = 8000
    box = (20.0, 20.0, 20.0)
    q = positions(n, box, RC, 0, np.float32, 110)
    kp_ref, lst_ref = ref_list(q, RC, box)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 111)
    nl = _handle(n, np.float32, 0, False, RC, box)
    nl.set_skin(0.3)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    _, b0 = nl.update_stats()
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == b0  # skipped
    nl.set_exclusions(pairs, n)
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == b0 + 1  # setting a table forces a build
    _assert_filtered(nl, kp_ref, lst_ref, pairs)
    nl.update(qd, sync=True)  # skipped: the filtered list stays
    assert nl.update_stats()[1] == b0 + 1
    _assert_filtered(nl, kp_ref, lst_ref, pairs)
    # update + forces captured once, replayed with positions moved below and beyond half the skin
    f = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nl.update(qd)
        nl.lj_forces(qd, wait=False, out=f)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nl.update(qd)
        nl.lj_forces(qd, wait=False, out=f)
    q2 = q.copy()
    q2[:, :3] = np.clip(q2[:, :3] + 0.4, 0.0, 19.999)  # past skin / 2: a build
    qd.copy_(torch.from_numpy(q2))
    g.replay()
    torch.cuda.synchronize()
    kr, lr = ref_list(q2, RC, box)
    _assert_filtered(nl, kr, lr, pairs)
    assert torch.isfinite(f).all()


@pytest.mark.gpu
def test_resort_relabels_the_table():
    torch = _torch()
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 120)
    kp_ref, lst_ref = ref_list(q, RC, BOX)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 121)
    nl = _handle(n, np.float32)
    nl.set_exclusions(pairs, n)
    qd = _build(nl, q)
    order = nl.cell_order().cpu().numpy().copy()
    vel = torch.arange(n, dtype=torch.int32, device="cuda")
    nl.resort(qd, vel)  # (two arrays: the table is relabelled once)
    torch.cuda.synchronize()
    assert np.array_equal(vel.cpu().numpy(), order)
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    pairs2 = inv[pairs.astype(np.int64)]
    off, ids = (t.cpu().numpy() for t in nl.exclusions())
    off_w, ids_w = table_csr(pairs2, n)
    assert np.array_equal(off, off_w) and np.array_equal(ids, ids_w)
    qp = q[order]
    nl.MakeNeighList(qd, n)
    kr, lr = ref_list(qp, RC, BOX)
    _assert_filtered(nl, kr, lr, pairs2)


@pytest.mark.gpu
def test_table_set_after_a_build_is_relabelled():
    """build (no table) -> set -> resort -> build: the table given in the order before the re-sort follows the particles;
    and a table replaced between a build and a re-sort is relabelled too."""
    torch = _torch()
    n = 20000
    q = positions(n, BOX, RC, 0, np.float32, 125)
    kp_ref, lst_ref = ref_list(q, RC, BOX)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 126)
    nl = _handle(n, np.float32)
    qd = _build(nl, q)
    nl.set_exclusions(pairs, n)
    order = nl.cell_order().cpu().numpy().copy()
    nl.resort(qd)
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    qp = q[order]
    nl.MakeNeighList(qd, n)
    kr, lr = ref_list(qp, RC, BOX)
    _assert_filtered(nl, kr, lr, inv[pairs.astype(np.int64)])
    # the table replaced (in the current order) after that build, then a re-sort
    pairs2 = mixed_pairs(kr, lr, n, 127)
    nl.set_exclusions(pairs2, n)
    order2 = nl.cell_order().cpu().numpy().copy()
    nl.resort(qd)
    torch.cuda.synchronize()
    inv2 = np.empty(n, dtype=np.int64)
    inv2[order2] = np.arange(n)
    nl.MakeNeighList(qd, n)
    kr2, lr2 = ref_list(qp[order2], RC, BOX)
    _assert_filtered(nl, kr2, lr2, inv2[pairs2.astype(np.int64)])


@pytest.mark.gpu
def test_captured_step_survives_a_resort():
    """update + forces captured once; resort (relabels the table), one forced update outside the graph, replays with moved
    positions: the list equals the oracle on the permuted positions minus the relabelled pairs (the table stays where the
    captured launches read it)."""
    torch = _torch()
    n = 8000
    box = (20.0, 20.0, 20.0)
    rng = np.random.default_rng(150)
    g = np.stack(np.meshgrid(*(np.arange(20),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # a jittered lattice:
    q = np.zeros((n, 4), dtype=np.float32)                                                   # no pair closer than ~0.5
    q[:, :3] = 0.5 + 0.9 * g + rng.uniform(-0.05, 0.05, size=(n, 3))
    q = q[rng.permutation(n)]
    kp_ref, lst_ref = ref_list(q, RC, box)
    pairs = mixed_pairs(kp_ref, lst_ref, n, 151)
    nl = _handle(n, np.float32, 0, False, RC, box)
    nl.set_skin(0.3)
    nl.set_exclusions(pairs, n)
    qd = torch.from_numpy(q).cuda()
    f = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    nl.update(qd, sync=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nl.update(qd)
        nl.lj_forces(qd, wait=False, out=f)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nl.update(qd)
        nl.lj_forces(qd, wait=False, out=f)
    g.replay()
    torch.cuda.synchronize()
    off0 = nl.exclusions()[0].data_ptr()
    order = nl.cell_order().cpu().numpy().copy()
    nl.resort(qd)
    nl.update(qd, sync=True)  # (forced: the re-sort)
    assert nl.exclusions()[0].data_ptr() == off0
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    relabelled = inv[pairs.astype(np.int64)]
    qp = q[order].copy()
    for step in range(2):
        qp[:, :3] += rng.uniform(-0.1, 0.1, size=(n, 3)).astype(np.float32) + np.float32(0.2 * (step + 1) - 0.2 * step)
        qd.copy_(torch.from_numpy(qp))
        b0 = nl.update_stats()[1]
        g.replay()
        torch.cuda.synchronize()
        assert nl.update_stats()[1] == b0 + 1  # the replayed update built
        kr, lr = ref_list(qp, RC, box)
        _assert_filtered(nl, kr, lr, relabelled, step)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
def test_lj_forces(dtype, full):
    torch = _torch()
    rc, box = 3.0, (30.0, 30.0, 30.0)
    q, _ = inputs.uniform_box(20000, dtype=dtype, seed=130, box=box)

    def lists(q):
        h = _po().build(q, rc, box).canonical()
        return h.key_pointer, h.sorted_list

    kp, lst = lists(q)
    rows = np.repeat(np.arange(len(q), dtype=np.int64), np.diff(kp))
    d = q[rows, :3].astype(np.float64) - q[lst.astype(np.int64), :3].astype(np.float64)
    close = np.zeros(len(q), dtype=bool)
    r2 = (d * d).sum(axis=1)
    close[rows[r2 <= 0.64]] = True
    close[lst[r2 <= 0.64]] = True
    q = np.ascontiguousarray(q[~close])
    n = len(q)
    kp, lst = lists(q)
    pairs = mixed_pairs(kp, lst, n, 131)

    def lj(kp, lst):
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
        cols = lst.astype(np.int64)
        d = q[rows, :3].astype(np.float64) - q[cols, :3].astype(np.float64)
        r2 = (d * d).sum(axis=1)
        s6 = (1.0 / r2) ** 3
        fr = 24.0 * (2.0 * s6 * s6 - s6) / r2
        out = np.zeros((n, 4))
        for c in range(3):
            np.add.at(out[:, c], rows, fr * d[:, c])
            np.add.at(out[:, c], cols, -fr * d[:, c])
        pe = 4.0 * (s6 * s6 - s6)
        np.add.at(out[:, 3], rows, 0.5 * pe)
        np.add.at(out[:, 3], cols, 0.5 * pe)
        return out, lj_pair_magnitudes(n, rows, cols, d, r2), lj_rows_off_the_band(n, rows, cols, r2, rc, dtype)

    _, kp_w, lst_w = remove_pairs(kp, lst, pairs)
    (want, S, off_band), plain = lj(kp_w, lst_w), lj(kp, lst)[0]
    nl = _handle(n, dtype, 0, full, rc, box)
    nl.set_exclusions(pairs, n)
    qd = _build(nl, q)
    got = nl.lj_forces(qd, 1.0, 1.0).cpu().numpy().astype(np.float64)
    scale = np.abs(want).max(axis=0)
    tol = 2e-4 if dtype == np.float32 else 1e-11
    assert np.all(np.abs(got - want) <= tol * scale), (np.abs(got - want) / scale).max(axis=0)
    assert np.abs(plain - want).max() > 100 * tol * scale.max()
    # and per particle and component within c u S (tests/test_lj_consumer.py), off the 64-ulp band of rc_force = rc
    check_lj(got, want, S, dtype, rows=off_band)


@pytest.mark.gpu
def test_errors():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    torch = _torch()
    n = 4000
    box = (20.0, 20.0, 20.0)
    q = positions(n, box, RC, 0, np.float32, 140)
    nl = _handle(n, np.float32, 0, False, RC, box)
    good = np.array([[0, 1], [2, 3]], dtype=np.int32)
    nl.set_exclusions(good, n)
    for bad, nn in (([[0, n]], n), ([[-1, 2]], n), ([[5, 5]], n), ([[0, 1]], n + 1)):
        with pytest.raises(NLError) as e:
            nl.set_exclusions(np.array(bad, dtype=np.int32), nn)
        assert e.value.code == NL_ERR_ARG
        off, ids = (t.cpu().numpy() for t in nl.exclusions())  # the old table is kept
        assert len(off) == n + 1 and np.array_equal(ids[:2], [1, 0])
    with pytest.raises(TypeError):
        nl.set_exclusions(np.zeros((3, 3), dtype=np.int32), n)
    with pytest.raises(ValueError):  # (an int64 index that an int32 cast would wrap onto particle 1)
        nl.set_exclusions(np.array([[0, 2**32 + 1]], dtype=np.int64), n)
    qd = torch.from_numpy(q).cuda()
    with pytest.raises(NLError) as e:  # a build of another particle count
        nl.MakeNeighList(qd, n - 1)
    assert e.value.code == NL_ERR_ARG
    with pytest.raises(NLError) as e:  # slab builds are out of scope
        nl.MakeNeighListSlab(qd, torch.arange(n, dtype=torch.int32, device="cuda"), n, 0, nl.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    nl.MakeNeighList(qd, n)
    assert nl.half_number_of_pairs() >= 0

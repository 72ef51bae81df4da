"""Builds whose ids are the input rows (BuildPlan::id_rows: no caller ids, no tilt, the row-wise binning): tmp_row and
sorted_gid are neither written nor read, sorted_row doubles as the compact id array, and the searches take a group's rows
from the staged ids.  Every list is compared, after the per-row sort, with the CPU oracle and with a second GPU build of
the same positions that passes the ids arange(n) explicitly (a slab build over the whole z range), which keeps the id
arrays apart.  The last tests are about the high plane of the hit words (written and read only where a stream has more
than 16 tiles): boxes that mix cells with and without high bits, and stale high-plane rows of an earlier build."""
import numpy as np
import pytest

from md_neighbor_list_amd import inputs, slab
from tests.util import canonical_csr

pytestmark = pytest.mark.gpu

RC = 3.3
EDGE = 3.385  # cell edge of the boxes below: mesh m = a box of m * EDGE a side


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def _box(mesh):
    return tuple(m * EDGE for m in mesh)


def _uniform(mesh, rho=1.0, dtype=np.float32, seed=1, n=None):
    box = _box(mesh)
    if n is None:
        n = int(round(rho * box[0] * box[1] * box[2]))
    q, box = inputs.uniform_box(n, dtype=dtype, seed=seed, box=box)
    assert slab.mesh_of(box, RC) == tuple(mesh)
    return q, box


def _handle(box, n_max, dtype=np.float32, full=False, pbc=False):
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    nl = NeighListGPU(RC, *box, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=pbc)
    nl.Initialize(n_max)
    return nl


def _build(nl, q, sync=True):
    t = _torch().from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(t, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return t


def _build_with_ids(nl, q, ids=None):
    """The same build with caller ids (arange(n) unless given): a slab build that owns every layer."""
    torch = _torch()
    n = len(q)
    gid = torch.arange(n, dtype=torch.int32, device="cuda") if ids is None else torch.from_numpy(ids.astype(np.int32)).cuda()
    nl.MakeNeighListSlab(torch.from_numpy(np.ascontiguousarray(q)).cuda(), gid, n, 0, nl.mesh_size[2])


def _result(nl, full=False):
    """(key_pointer, counts, canonical list, checksum) of the last build, on the host."""
    if full:
        kp, lst, cnt = (t.cpu().numpy() for t in nl.full_csr())
    else:
        kp, lst, cnt = (t.cpu().numpy() for t in (nl.key_pointer(), nl.sorted_list(), nl.half_number_of_partners()))
    return kp, cnt, canonical_csr(kp, lst), nl.list_checksum()


def _full_of(ref):
    """(key_pointer, counts, canonical list) of the full list that holds both directions of the half list `ref`."""
    n = len(ref.key_pointer) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ref.key_pointer))
    lst = ref.sorted_list.astype(np.int64)
    i, j = np.concatenate([rows, lst]), np.concatenate([lst, rows])
    order = np.lexsort((j, i))
    cnt = np.bincount(i, minlength=n)
    return np.concatenate([[0], np.cumsum(cnt)]), cnt, j[order].astype(np.int32)


def _check_oracle(nl, ref, full=False):
    kp, cnt, lst, cs = _result(nl, full)
    if full:
        want_kp, want_cnt, want_lst = _full_of(ref)
    else:
        c = ref.canonical()
        want_kp, want_cnt, want_lst = ref.key_pointer, ref.number_of_partners, c.sorted_list
        assert nl.half_number_of_pairs() == ref.npairs
        assert cs == (ref.hash(), ref.npairs)
    assert np.array_equal(kp, want_kp)
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(lst, want_lst)


def _check_same(nl, other, full=False):
    a, b = _result(nl, full), _result(other, full)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]


def _check(q, box, dtype=np.float32, full=False, pbc=False, ref=None, nl=None):
    """One build without ids on `nl` (a new handle unless given) against the oracle and against the build with ids."""
    nl = nl or _handle(box, len(q), dtype, full, pbc)
    _build(nl, q)
    _check_oracle(nl, ref if ref is not None else _po().build(q, RC, box), full)
    other = _handle(box, len(q), dtype, full, pbc)
    _build_with_ids(other, q)
    _check_same(nl, other, full)
    return nl


# ------------------------------------------------------------------------------------------------ 1. basic shapes
@pytest.mark.parametrize("mesh,n", [((3, 3, 3), None), ((5, 4, 3), None), ((3, 3, 3), 1), ((3, 3, 3), 2), ((6, 6, 6), 8193)])
def test_basic_shapes(mesh, n):
    """fp32 half list at rho = 1: the smallest mesh of the id-class path, a non-cubic one, one and two particles, and
    three binning chunks (8193 particles at 4096 a chunk)."""
    q, box = _uniform(mesh, seed=3, n=n)
    if n == 2:
        q[1, :3] = q[0, :3] + np.float32(0.5)  # a pair
    nl = _check(q, box)
    if n is None:
        assert nl.build_info()["id_classes"] == 2 and nl.build_info()["masks"]


# ------------------------------------------------------------------------------------------------ 2. other paths
def test_full_list():
    q, box = _uniform((5, 4, 3), seed=4)
    _check(q, box, full=True)


def test_fp64():
    q, box = _uniform((5, 4, 3), dtype=np.float64, seed=5)
    _check(q, box, dtype=np.float64)


def test_minimum_image():
    from tests.test_periodic_axes import positions, reference

    box = _box((5, 4, 3))
    q = positions(2337, box, RC, 7, np.float32, seed=6)
    _check(q, box, pbc=True, ref=reference(q, RC, box, 7))


def test_sparse_box():
    """rho = 0.5: the 2-wave COUNT sweep and the 1-wave expansion."""
    q, box = _uniform((5, 4, 3), rho=0.5, seed=7)
    nl = _check(q, box)
    assert nl.build_info()["small_cells"]


def test_dense_box():
    """rho = 1.2: streams past one LDS batch (fine rows, or hit masks per batch)."""
    q, box = _uniform((5, 4, 3), rho=1.2, seed=8)
    nl = _check(q, box)
    assert nl.build_info()["id_classes"] == 0


# ------------------------------------------------------------------------------------------------ 3. cell order
def test_cell_order():
    """sorted_state(), nl_get_cell_order and nl_resort after a build without ids: the order is a permutation that puts
    every particle in the cell the reference's hash gives it."""
    torch = _torch()
    q, box = _uniform((5, 4, 3), seed=9)
    cells, mesh = _po().cells(q, RC, box)
    nl = _handle(box, len(q))
    _build(nl, q)
    assert nl.build_info()["fine_rows"] == 0
    cell_start, sorted_row = (t.cpu().numpy() for t in nl.sorted_state())
    order = nl.cell_order().cpu().numpy()
    assert np.array_equal(order, sorted_row)
    assert cell_start[0] == 0 and cell_start[-1] == len(q) and np.all(np.diff(cell_start) >= 0)
    assert np.array_equal(np.sort(order), np.arange(len(q)))
    cell_of_slot = np.repeat(np.arange(len(cell_start) - 1), np.diff(cell_start))
    assert np.array_equal(cells[order], cell_of_slot)
    a = torch.arange(len(q), dtype=torch.int32, device="cuda")
    nl.resort(a)
    assert np.array_equal(a.cpu().numpy(), order)


# ------------------------------------------------------------------------------------------------ 4. alternating ids
def test_alternating_ids_on_one_handle():
    """Without ids, with shuffled ids, without again, on one handle: no stale alias and no stale id array."""
    q, box = _uniform((5, 4, 3), seed=10)
    n = len(q)
    ref = _po().build(q, RC, box)
    perm = np.random.default_rng(11).permutation(n)
    ref_perm = _po().build(q[np.argsort(perm)], RC, box)  # particle i of q carries id perm[i]: the list of the ids
    nl = _handle(box, n)
    for with_ids in (False, True, False, True, False):
        if with_ids:
            _build_with_ids(nl, q, perm)
            kp, cnt, lst, _ = _result(nl)
            # rows stay the caller's rows; entries are ids: compare as a set of id pairs
            rows = perm[np.repeat(np.arange(n), np.diff(kp))]
            got = np.sort((np.minimum(rows, lst).astype(np.int64) << 32) | np.maximum(rows, lst))
            c = ref_perm.canonical()
            want_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(c.key_pointer))
            assert np.array_equal(got, np.sort((want_rows << 32) | c.sorted_list))
            assert np.all(lst > rows)  # the half-list rule on ids
        else:
            _build(nl, q)
            _check_oracle(nl, ref)


# ------------------------------------------------------------------------------------------------ 5. rerun, two-pass
def test_rerun_on_the_two_pass_binning():
    """A dense slab in one row of x-cells overflows its bucket: finish() runs the build again on the two-pass binning
    (k_bin_rows, k_bin_scatter), still without ids."""
    rc, box = RC, (40.0, 40.0, 40.0)
    q0, _ = inputs.uniform_box(30000, dtype=np.float32, seed=71, box=box)
    rng = np.random.default_rng(72)
    m = slab.mesh_of(box, rc)
    s = np.zeros((600, 4), dtype=np.float32)
    s[:, 0] = rng.uniform(0.0, box[0] * (1 - 1e-6), 600)
    s[:, 1] = (3 + rng.uniform(0.05, 0.95, 600)) * box[1] / m[1]
    s[:, 2] = (5 + rng.uniform(0.05, 0.95, 600)) * box[2] / m[2]
    q = np.concatenate([q0, s])
    nl = _handle(box, len(q))
    _build(nl, q0)
    first = nl.build_stats()
    assert first["row_overflow_reruns"] == 0 and first["cap_row"] > 0
    _check(q, box, nl=nl)
    assert nl.build_stats()["row_overflow_reruns"] == 1


# ------------------------------------------------------------------------------------------------ 6. graph, update
def test_graph_replay_and_update():
    torch = _torch()
    q, box = _uniform((5, 4, 3), seed=12)
    q2, _ = _uniform((5, 4, 3), seed=13)
    n = len(q)
    refs = [_po().build(x, RC, box) for x in (q, q2)]
    nl = _handle(box, n)
    nl.set_graph(True)
    qd = torch.from_numpy(q).cuda()
    for k in (0, 1, 0):  # the capture and two replays
        qd.copy_(torch.from_numpy((q, q2)[k]))
        nl.MakeNeighList(qd, n, sync=False)
        nl.synchronize()
        _check_oracle(nl, refs[k])
    gid = torch.arange(n, dtype=torch.int32, device="cuda")  # a build with ids: another key, captured anew
    nl.MakeNeighListSlab(qd, gid, n, 0, nl.mesh_size[2], sync=False)
    nl.synchronize()
    _check_oracle(nl, refs[0])
    nl.MakeNeighList(qd, n, sync=False)
    nl.synchronize()
    _check_oracle(nl, refs[0])
    # one update after a build without ids
    up = _handle(box, n)
    up.set_skin(0.4)
    up.update(qd, sync=True)
    _check_oracle(up, refs[0])
    moved = q.copy()
    moved[:50, 0] = np.clip(moved[:50, 0] + 0.5, 0, np.nextafter(np.float32(box[0]), np.float32(0)))  # past skin / 2
    qd.copy_(torch.from_numpy(moved))
    up.update(qd, sync=True)
    assert up.update_stats() == (2, 2)
    _check_oracle(up, _po().build(moved, RC, box))


# ------------------------------------------------------------------------------------------------ 7. out of the box
def test_positions_outside_the_box():
    """Particles up to one box length outside the box on every axis (the +-m wrap of the cell index; the open box keeps
    their coordinates)."""
    q, box = _uniform((5, 4, 3), seed=14)
    rng = np.random.default_rng(15)
    idx = rng.choice(len(q), 300, replace=False)
    for k, d in enumerate((0, 1, 2)):
        lo, hi = idx[100 * k:100 * k + 50], idx[100 * k + 50:100 * k + 100]
        q[lo, d] = (-rng.uniform(0.0, 0.999, 50) * box[d]).astype(np.float32)
        q[hi, d] = ((1.0 + rng.uniform(0.0, 0.999, 50)) * box[d]).astype(np.float32)
    _check(q, box)


# ------------------------------------------------------------------------------------------------ 8, 9. the high plane
def _stream_tiles(q, box):
    """Tiles (64 slots) of every cell's stencil stream: the particles of its 27 cells (wrapped)."""
    cells, mesh = _po().cells(q, RC, box)
    mesh = tuple(int(m) for m in mesh)
    cnt = np.bincount(cells, minlength=int(np.prod(mesh))).reshape(mesh[2], mesh[1], mesh[0])
    stream = sum(np.roll(cnt, (dz, dy, dx), axis=(0, 1, 2)) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return (stream + 63) // 64


MIXED_SEED = 21


@pytest.mark.parametrize("rho,kind", [(0.8, "none"), (1.0, "mixed"), (1.03, "most")])
def test_high_plane_mixed_cells(rho, kind):
    """Streams of at most 16 tiles have no high bits.  A 4 x 4 x 4 mesh at rho = 1 mixes cells with and without them;
    at rho = 0.8 no cell has them, at rho = 1.03 nearly every cell has (still one LDS batch)."""
    q, box = _uniform((4, 4, 4), rho=rho, seed=MIXED_SEED)
    tiles = _stream_tiles(q, box)
    assert tiles.max() <= 20  # one LDS batch
    if kind == "none":
        assert np.all(tiles <= 16)
    elif kind == "mixed":
        assert np.any(tiles <= 16) and np.any(tiles > 16)
    else:
        assert np.mean(tiles > 16) > 0.75
    nl = _check(q, box)
    assert nl.build_info()["id_classes"] == 2


def test_stale_high_plane():
    """A build that writes every high-plane row, then another box of the same n on the same handle: rows whose high
    plane the second build leaves out must not pick up the first build's bytes."""
    q1, box = _uniform((4, 4, 4), rho=1.03, seed=MIXED_SEED)
    nl = _handle(box, len(q1))
    _build(nl, q1)
    _check_oracle(nl, _po().build(q1, RC, box))
    for seed in (22, 23):
        q2, _ = _uniform((4, 4, 4), seed=seed, n=len(q1))
        _check(q2, box, nl=nl)
    q3, _ = _uniform((4, 4, 4), seed=24)  # fewer particles: cells without high bits among them
    _check(q3, box, nl=nl)

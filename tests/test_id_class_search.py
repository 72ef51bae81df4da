"""The half-list search by id class (NL_IDCLASS; k_sweep_class_f32, k_bin_cells<IDC>, k_fill_masks<IDC>): each cell's
particles sorted by id class, the stencil staged class-major, lower-class partners never tested and higher-class
partners tested without the id compare.  Every list is compared with the CPU oracle after the canonical sort, with the
path forced to 2 and 4 classes and forced off; the plan must leave it out wherever it is not exact."""
import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.util import canonical_csr

pytestmark = pytest.mark.gpu

RC = 3.3
CLASSES = ("0", "2", "4")


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def _handle(monkeypatch, c, q, box, full=False, pbc=False, graph=False):
    from md_neighbor_list_amd import NeighListGPU

    monkeypatch.setenv("NL_IDCLASS", c)  # (read when the handle is created)
    if graph:
        monkeypatch.setenv("NL_GRAPH", "1")
    nl = NeighListGPU(RC, *box, dtype=_torch().float32, full_list=full, minimum_image=pbc)
    nl.Initialize(len(q))
    return nl


def _check(nl, q, box, c):
    ref = _po().build(q, RC, box)
    kp = nl.key_pointer().cpu().numpy()
    assert nl.half_number_of_pairs() == ref.npairs
    assert np.array_equal(nl.half_number_of_partners().cpu().numpy(), ref.number_of_partners)
    assert np.array_equal(kp, ref.key_pointer)
    assert np.array_equal(canonical_csr(kp, nl.sorted_list().cpu().numpy()), ref.canonical().sorted_list)
    assert nl.list_checksum() == (ref.hash(), ref.npairs)
    assert nl.build_info()["id_classes"] == int(c), nl.build_info()


def _build(nl, q):
    nl.MakeNeighList(_torch().from_numpy(q).cuda(), len(q))


def _spatial_ids(q, box):
    """The same particles with ids in cell order (z, y, x): ids correlate with space, so classes are spatial slabs."""
    m = [int(b / RC) for b in box]
    c = [np.minimum((q[:, d] / (box[d] / m[d])).astype(np.int64), m[d] - 1) for d in range(3)]
    return np.ascontiguousarray(q[np.lexsort((c[0], c[1], c[2]))])


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("ids", ["random", "spatial"])
def test_parity(monkeypatch, c, ids):
    q, box = inputs.uniform_box(36000, dtype=np.float32, seed=7, box=(34.2, 34.2, 34.2))
    if ids == "spatial":
        q = _spatial_ids(q, box)
    nl = _handle(monkeypatch, c, q, box)
    _build(nl, q)
    assert nl.build_info()["masks"] and not nl.build_info()["small_cells"]
    _check(nl, q, box, c)


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("n", [33001, 40961, 49152])
def test_n_not_a_power_of_two(monkeypatch, c, n):
    """The last class is short (33001, 40961: one particle in the top class of 2^16 / 2^14 ids) or a power of two
    wide (49152 = 3 * 2^14).  11^3 cells: 25 to 37 particles a cell."""
    q, box = inputs.uniform_box(n, dtype=np.float32, seed=n, box=(37.0, 37.0, 37.0))
    nl = _handle(monkeypatch, c, q, box)
    _build(nl, q)
    _check(nl, q, box, c)


@pytest.mark.parametrize("c", CLASSES)
def test_clustered_cells_take_the_batched_search(monkeypatch, c):
    """A few cells hold several hundred particles: their streams exceed the LDS buffer, so k_sweep_list_f32 and
    k_fill_list take them, next to cells of the class search."""
    rng = np.random.default_rng(5)
    q, box = inputs.uniform_box(30000, dtype=np.float32, seed=9, box=(34.2, 34.2, 34.2))
    for centre in ((5.0, 5.0, 5.0), (20.0, 12.0, 28.0)):
        q[rng.choice(len(q), 700, replace=False), :3] = (np.asarray(centre) + rng.uniform(0, 2.5, (700, 3))).astype(np.float32)
    q = np.ascontiguousarray(q[rng.permutation(len(q))])
    nl = _handle(monkeypatch, c, q, box)
    for _ in range(6):  # (past the builds that launch the list kernels unconditionally)
        _build(nl, q)
        _check(nl, q, box, c)
    assert nl.build_stats()["list_launched"]


@pytest.mark.parametrize("c", ["2", "4"])
def test_exclusions_and_type_cutoffs(monkeypatch, c):
    from tests.test_exclusions import mixed_pairs, remove_pairs
    from tests.test_type_cutoffs import type_filter

    q, box = inputs.uniform_box(36000, dtype=np.float32, seed=11, box=(34.2, 34.2, 34.2))
    n = len(q)
    ref = _po().build(q, RC, box).canonical()
    pairs = mixed_pairs(ref.key_pointer, ref.sorted_list, n, 3)
    counts, kp_ex, lst_ex = remove_pairs(ref.key_pointer, ref.sorted_list, pairs)
    rng = np.random.default_rng(4)
    types = rng.integers(0, 2, n).astype(np.int32)
    rcm = np.array([[3.3, 2.7], [2.7, 3.0]])
    _, kp_ty, lst_ty = type_filter(ref.key_pointer, ref.sorted_list, q, RC, box, 0, np.float32, types, rcm)
    for kind, (kp_want, lst_want) in (("ex", (kp_ex, lst_ex)), ("ty", (kp_ty, lst_ty))):
        nl = _handle(monkeypatch, c, q, box)
        if kind == "ex":
            nl.set_exclusions(pairs, n)
        else:
            nl.set_type_cutoffs(types, rcm)
        _build(nl, q)
        assert nl.build_info()["id_classes"] == int(c)
        kp = nl.key_pointer().cpu().numpy()
        assert np.array_equal(kp, kp_want), kind
        assert np.array_equal(canonical_csr(kp, nl.sorted_list().cpu().numpy()), lst_want), kind


@pytest.mark.parametrize("c", CLASSES)
def test_update_and_graph_replay(monkeypatch, c):
    torch = _torch()
    q, box = inputs.uniform_box(36000, dtype=np.float32, seed=13, box=(34.2, 34.2, 34.2))
    nl = _handle(monkeypatch, c, q, box, graph=True)
    nl.set_skin(0.4)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    _check(nl, q, box, c)
    q2 = q.copy()
    q2[:100, 0] = np.clip(q2[:100, 0] + 0.5, 0, np.nextafter(np.float32(box[0]), np.float32(0)))  # past skin / 2: a rebuild
    qd.copy_(torch.from_numpy(q2))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 2)
    _check(nl, q2, box, c)
    # plain builds replayed from the captured graph
    nl2 = _handle(monkeypatch, c, q, box, graph=True)
    for qq in (q, q2, q):
        qd.copy_(torch.from_numpy(qq))
        nl2.MakeNeighList(qd, len(qq), sync=False)
        nl2.synchronize()
        _check(nl2, qq, box, c)


def test_the_plan_falls_back(monkeypatch):
    """Full lists, periodic axes, slab builds (caller ids) and sparse boxes keep the plain search."""
    import torch

    from md_neighbor_list_amd import NeighListGPU

    q, box = inputs.uniform_box(36000, dtype=np.float32, seed=7, box=(34.2, 34.2, 34.2))
    qd = torch.from_numpy(q).cuda()
    nl = _handle(monkeypatch, "2", q, box, full=True)
    nl.MakeNeighList(qd, len(q))
    assert nl.build_info()["masks"] and nl.build_info()["id_classes"] == 0
    nl = _handle(monkeypatch, "2", q, box)
    nl.set_periodic(True, axes="x")
    nl.MakeNeighList(qd, len(q))
    assert nl.build_info()["id_classes"] == 0
    nl = _handle(monkeypatch, "2", q, box, pbc=True)
    nl.MakeNeighList(qd, len(q))
    assert nl.build_info()["id_classes"] == 0
    # a slab build: caller ids (layers 2..5 owned, ghosts at 1 and 6)
    m = int(box[2] / RC)
    iz = np.minimum((q[:, 2] / (box[2] / m)).astype(np.int64), m - 1)
    own, glo, ghi = (np.nonzero(sel)[0] for sel in ((iz >= 2) & (iz < 6), iz == 1, iz == 6))
    order = np.concatenate([own, glo, ghi])
    nl = NeighListGPU(RC, *box, dtype=torch.float32)
    nl.Initialize(len(order))
    nl.MakeNeighListSlab(torch.from_numpy(q[order]).cuda(), torch.from_numpy(order.astype(np.int32)).cuda(), len(own), 2, 6)
    assert nl.build_info()["id_classes"] == 0
    # a sparse box (the 2-wave instances)
    qs, boxs = inputs.uniform_box(12000, dtype=np.float32, seed=3, box=(34.2, 34.2, 34.2))
    nl = _handle(monkeypatch, "2", qs, boxs)
    _build(nl, qs)
    assert nl.build_info()["small_cells"] and nl.build_info()["id_classes"] == 0
    _check(nl, qs, boxs, "0")

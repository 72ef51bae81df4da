"""The reach cull of the id-class search (BuildPlan::cull, NL_CULL; cls_cull in nl_kernels.hpp): the COUNT sweep drops
from a cell's staged stream every partner that lies farther than the cut-off from the bounding box of the cell's own
particles, compacts the stream, and leaves the ballots to the expansion, which compacts the ids the same way.  Counts,
key_pointer and the set of partners in every row must stay what they were: every list here is compared with the CPU
oracle after the canonical sort, with the cull on (NL_CULL unset) and off (NL_CULL=0), and build_info()["reach_cull"]
is asserted.

Shapes: the smallest that take the path (more than 19.6 particles per cell, so that the 4-wave kernels run) and reach
the edge in question; each case builds a few thousand to 36 000 particles once."""
import functools

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests import cutoff_util as cu
from tests.util import canonical_csr

pytestmark = pytest.mark.gpu

RC = 3.3
BOX10 = (34.2, 34.2, 34.2)  # 10 x 10 x 10 cells
CULL = (True, False)
DELTA = 2.0 ** -20  # CULL_DELTA of nl_kernels.hpp


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _uniform(n, seed, box):
    q, _ = inputs.uniform_box(n, dtype=np.float32, seed=seed, box=box)
    q.setflags(write=False)
    return q


_REFS = {}


def _ref(q, box):
    """The oracle's list of q, built once per input."""
    key = (q.tobytes(), tuple(box))
    if key not in _REFS:
        ref = _po().build(q, RC, box)
        _REFS[key] = (ref, ref.canonical().sorted_list)
    return _REFS[key]


def _handle(monkeypatch, cull, n, box, **env):
    from md_neighbor_list_amd import NeighListGPU

    monkeypatch.delenv("NL_CULL", raising=False)
    if not cull:
        monkeypatch.setenv("NL_CULL", "0")  # (read when the handle is created, like NL_IDCLASS)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nl = NeighListGPU(RC, *box, dtype=_torch().float32)
    nl.Initialize(n)
    return nl


def _check(nl, q, box, cull, classes=2, wide=False):
    ref, lst = _ref(q, box)
    info = nl.build_info()
    assert info["masks"] and info["id_classes"] == classes and info["reach_cull"] == cull, info
    kp = (nl.key_pointer64() if wide else nl.key_pointer()).cpu().numpy()
    assert nl.half_number_of_pairs() == ref.npairs
    assert np.array_equal(nl.half_number_of_partners().cpu().numpy(), ref.number_of_partners)
    assert np.array_equal(kp, ref.key_pointer)
    assert np.array_equal(canonical_csr(kp, nl.sorted_list().cpu().numpy()), lst)
    assert nl.list_checksum() == (ref.hash(), ref.npairs)


def _build(nl, q, sync=True):
    nl.MakeNeighList(_torch().from_numpy(np.array(q)).cuda(), len(q), sync=sync)


def _spatial_ids(q, box):
    """The same particles with ids in cell order (z, y, x): the classes are slabs, so most cells lack one."""
    m = cu.mesh(box)
    c = [np.minimum((q[:, d] / (box[d] / m[d])).astype(np.int64), m[d] - 1) for d in range(3)]
    return np.ascontiguousarray(q[np.lexsort((c[0], c[1], c[2]))])


def _mesh_box(m):
    return tuple(k * RC * 1.03 for k in m)


# ------------------------------------------------------------------------------------------ the layout on the CPU

def kept_layout(q, box, delta=DELTA):
    """Per non-empty cell (kept slots of its stream, compacted start of class 1), in float64: what cls_cull arrives at up
    to the rounding of G2.  The stencil wraps and does not shift (open box), each of the 27 cells once (mesh >= 3)."""
    m = np.array(cu.mesh(box))
    c, _ = cu.stored(q, box, RC, 0)
    n = len(q)
    shift = 0
    while (n - 1) >> shift >= 2:
        shift += 1
    cls = np.arange(n) >> shift
    key = (c[:, 2] * m[1] + c[:, 1]) * m[0] + c[:, 0]
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(m.prod() + 1))
    p = q[:, :3].astype(np.float64)
    out = []
    for cell in range(int(m.prod())):
        own = order[start[cell]:start[cell + 1]]
        if len(own) == 0:
            continue
        lo, hi = p[own].min(axis=0), p[own].max(axis=0)
        cx, cy, cz = cell % m[0], cell // m[0] % m[1], cell // (m[0] * m[1])
        js = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = ((cz + dz) % m[2] * m[1] + (cy + dy) % m[1]) * m[0] + (cx + dx) % m[0]
                    js.append(order[start[k]:start[k + 1]])
        js = np.concatenate(js)
        gap = np.maximum(np.maximum(lo - p[js], p[js] - hi), 0.0)
        kept = ~((gap * gap).sum(axis=1) > RC * RC * (1.0 + delta))
        out.append((int(kept.sum()), int((kept & (cls[js] == 0)).sum())))
    return np.array(out)


# ------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("ids", ["random", "spatial"])
def test_parity(monkeypatch, cull, ids):
    q = _uniform(36000, 7, BOX10)
    if ids == "spatial":
        q = _spatial_ids(q, BOX10)
    nl = _handle(monkeypatch, cull, len(q), BOX10)
    _build(nl, q)
    _check(nl, q, BOX10, cull)


@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("m", [(3, 3, 3), (3, 4, 5), (5, 5, 5)])
def test_small_meshes(monkeypatch, cull, m):
    """Every stencil wraps: the wrapped neighbours are staged where they are, out of everyone's reach."""
    box = _mesh_box(m)
    q = _uniform(36 * m[0] * m[1] * m[2], 100 + sum(m), box)
    nl = _handle(monkeypatch, cull, len(q), box)
    _build(nl, q)
    _check(nl, q, box, cull)


LONELY_BOX = (17.0, 17.0, 17.0)  # 5 x 5 x 5 cells of edge 3.4


@functools.lru_cache(maxsize=None)
def lonely_cloud():
    """36 particles per cell, but one particle alone in each of the 8 cells with odd indices (box = point: the cull test
    of such a cell is the pair test), and 40 partners of each in the cells around it at r2 = rc2 + k ulp, k in [-32, 32]
    before the partner is rounded to fp32.  Returns (q, lonely ids, partner ids, their centres' ids)."""
    rng = np.random.default_rng(20)
    L, ms = np.array(LONELY_BOX), 3.4
    odd = lambda x: np.all(np.floor(x / ms).astype(int) % 2 == 1, axis=1)  # noqa: E731
    bg = rng.uniform(0, 1, (36 * 125, 3)) * L
    bg = bg[~odd(bg)]
    cen = np.array([(x, y, z) for x in (1, 3) for y in (1, 3) for z in (1, 3)]) * ms + rng.uniform(0.3, 3.1, (8, 3))
    cen = cen.astype(np.float32).astype(np.float64)
    ulp = float(np.spacing(np.float32(RC * RC)))
    who = np.repeat(np.arange(8), 80)
    d = rng.normal(size=(len(who), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.sqrt(RC * RC + rng.integers(-32, 33, len(who)) * ulp)
    par = cen[who] + d * r[:, None]
    ok = ~odd(par)  # (a partner inside the lonely cell would end its solitude)
    who, par = who[ok][:320], par[ok][:320]
    pos = np.concatenate([cen, par, bg]).astype(np.float32)
    perm = rng.permutation(len(pos))
    q = np.zeros((len(pos), 4), dtype=np.float32)
    q[perm, :3] = pos
    q.setflags(write=False)
    return q, perm[:8], perm[8:8 + len(par)], perm[:8][who]


def test_the_lonely_cloud_sits_on_the_cutoff():
    """(CPU) one particle per odd cell, and its partners on both sides of the cut-off within 32 ulp."""
    q, lonely, par, cen = lonely_cloud()
    c, _ = cu.stored(q, LONELY_BOX, RC, 0)
    m = np.array(cu.mesh(LONELY_BOX))
    assert tuple(m) == (5, 5, 5)
    key = (c[:, 2] * 5 + c[:, 1]) * 5 + c[:, 0]
    assert np.all(np.bincount(key, minlength=125)[key[lonely]] == 1)
    assert np.all(np.any(c[par] != c[cen], axis=1))
    r2, visited = cu.rule_r2(q, cen, par, LONELY_BOX, RC, 0)
    near = cu.near_cutoff(r2, RC, ulps=32) & visited
    acc = cu.accepted(q, cen, par, LONELY_BOX, RC, 0)
    assert (near & acc).sum() >= 40 and (near & ~acc).sum() >= 40, ((near & acc).sum(), (near & ~acc).sum())
    assert np.any(near & (r2 == np.float32(RC * RC)))  # and some exactly on it


@pytest.mark.parametrize("cull", CULL)
def test_last_bit_one_particle_cells(monkeypatch, cull):
    q, lonely, par, cen = lonely_cloud()
    acc = cu.accepted(q, cen, par, LONELY_BOX, RC, 0)
    assert acc.any() and (~acc).any()
    # the brute force by the header's rule agrees with the oracle on this cloud (half list: j > i)
    cnt, kp_b, lst_b = cu.brute_force(q, LONELY_BOX, RC, 0)
    rows = np.repeat(np.arange(len(cnt)), cnt)
    ref, lst = _ref(q, LONELY_BOX)
    assert np.array_equal(lst_b[lst_b > rows], lst)
    nl = _handle(monkeypatch, cull, len(q), LONELY_BOX)
    _build(nl, q)
    _check(nl, q, LONELY_BOX, cull)
    # no constructed pair left out, none let in
    kp = nl.key_pointer().cpu().numpy()
    got = canonical_csr(kp, nl.sorted_list().cpu().numpy())
    lo, hi = np.minimum(cen, par), np.maximum(cen, par)
    has = np.array([b in got[kp[a]:kp[a + 1]] for a, b in zip(lo, hi)])
    assert np.array_equal(has, acc)


@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("classes", [("rand", "corner", "zplane"), tuple(cu.OUTSIDE)])
def test_last_bit_and_outside_the_box(monkeypatch, cull, classes):
    """Pairs at rc (1 + k ulp) at random places, across cell corners and along z; and particles a box length below 0 and
    above L, filed into the edge cells, with their partners around them (the box of an edge cell then reaches outside)."""
    rng = np.random.default_rng(len(classes[0]))
    q, pairs = cu.cloud(cu.BOX, RC, np.float32, 0, classes, rng, per_cell=30.0, with_pairs=True)
    r2, visited = cu.rule_r2(q, pairs["a"], pairs["b"], cu.BOX, RC, 0)
    near = cu.near_cutoff(r2, RC) & visited
    acc = cu.accepted(q, pairs["a"], pairs["b"], cu.BOX, RC, 0)
    assert (near & acc).sum() >= 100 and (near & ~acc).sum() >= 100
    if classes[0] in cu.OUTSIDE:
        assert (q[:, :3] < 0).any() and (q[:, :3] > np.array(cu.BOX)).any()
    nl = _handle(monkeypatch, cull, len(q), cu.BOX)
    _build(nl, q)
    _check(nl, q, cu.BOX, cull)


TILE_BOX = _mesh_box((5, 5, 5))
TILE_SEEDS = tuple(range(300, 316))


def test_the_tile_edge_seeds_reach_the_edges():
    """(CPU) over the 16 boxes some cell's kept count, and some cell's compacted class-1 start, is a multiple of 64, and
    some is one short of it: the survivors end on a tile's last lane and begin a tile."""
    kept, start1 = [], []
    for seed in TILE_SEEDS:
        lay = kept_layout(_uniform(4500, seed, TILE_BOX), TILE_BOX)
        kept.append(lay[:, 0]), start1.append(lay[:, 1])
    kept, start1 = np.concatenate(kept), np.concatenate(start1)
    assert kept.max() <= 1216 and kept.min() > 0
    for v in (kept, start1):
        assert np.any(v % 64 == 0) and np.any(v % 64 == 63), np.bincount(v % 64, minlength=64)


@pytest.mark.parametrize("cull", CULL)
def test_tile_edges(monkeypatch, cull):
    nl = _handle(monkeypatch, cull, 4500, TILE_BOX)
    for seed in TILE_SEEDS:
        q = _uniform(4500, seed, TILE_BOX)
        _build(nl, q)
        _check(nl, q, TILE_BOX, cull)


@pytest.mark.parametrize("cull", CULL)
def test_clustered_cells_take_the_list_kernels(monkeypatch, cull):
    """Streams beyond the LDS buffer (decided on the staged length) go to k_sweep_list_f32 / k_fill_list, next to culled
    cells; and cells whose stream leaves no room for the ballots keep every slot."""
    rng = np.random.default_rng(5)
    q = _uniform(30000, 9, BOX10).copy()
    for centre, k in (((5.0, 5.0, 5.0), 700), ((20.0, 12.0, 28.0), 700), ((27.0, 27.0, 8.0), 330)):
        q[rng.choice(len(q), k, replace=False), :3] = (np.asarray(centre) + rng.uniform(0, 2.5, (k, 3))).astype(np.float32)
    q = np.ascontiguousarray(q[rng.permutation(len(q))])
    nl = _handle(monkeypatch, cull, len(q), BOX10)
    for _ in range(6):  # (past the builds that launch the list kernels unconditionally)
        _build(nl, q)
        _check(nl, q, BOX10, cull)
    assert nl.build_stats()["list_launched"]


@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("n", [20500, 36000])
def test_both_row_batches(monkeypatch, cull, n):
    """20.5 particles per cell: the expansion that loads 12 rows a wave; 36: the one that loads 24."""
    q = _uniform(n, 31, BOX10)
    nl = _handle(monkeypatch, cull, n, BOX10)
    _build(nl, q)
    _check(nl, q, BOX10, cull)


@pytest.mark.parametrize("cull", CULL)
def test_four_classes(monkeypatch, cull):
    q = _uniform(36000, 7, BOX10)
    nl = _handle(monkeypatch, cull, len(q), BOX10, NL_IDCLASS="4")
    _build(nl, q)
    _check(nl, q, BOX10, cull, classes=4)


@pytest.mark.parametrize("cull", CULL)
def test_wide_offsets(monkeypatch, cull):
    q = _uniform(36000, 7, BOX10)
    nl = _handle(monkeypatch, cull, len(q), BOX10, NL_OFFSET_WIDTH="64")
    _build(nl, q)
    assert nl.build_info()["offset_bits"] == 64
    _check(nl, q, BOX10, cull, wide=True)


@pytest.mark.parametrize("cull", CULL)
def test_graph_replay_with_two_inputs(monkeypatch, cull):
    torch = _torch()
    qa, qb = _uniform(36000, 7, BOX10), _uniform(36000, 8, BOX10)
    nl = _handle(monkeypatch, cull, 36000, BOX10, NL_GRAPH="1")
    qd = torch.from_numpy(qa.copy()).cuda()
    for q in (qa, qb, qa, qb):
        qd.copy_(torch.from_numpy(q.copy()))
        nl.MakeNeighList(qd, len(q), sync=False)
        nl.synchronize()
        _check(nl, q, BOX10, cull)


@pytest.mark.parametrize("cull", CULL)
def test_a_list_grown_after_the_search(monkeypatch, cull):
    """The expansion runs again on the grown list, with the ballots of the COUNT sweep it belongs to."""
    q = _uniform(36000, 7, BOX10)
    nl = _handle(monkeypatch, cull, len(q), BOX10)
    nl.set_capacity(1000)
    _build(nl, q, sync=True)
    _check(nl, q, BOX10, cull)


@pytest.mark.parametrize("cull", CULL)
def test_a_skipped_update_and_a_rebuild(monkeypatch, cull):
    torch = _torch()
    q = _uniform(36000, 13, BOX10)
    nl = _handle(monkeypatch, cull, len(q), BOX10)
    nl.set_skin(0.4)
    qd = torch.from_numpy(q.copy()).cuda()
    nl.update(qd, sync=True)
    _check(nl, q, BOX10, cull)
    nl.update(qd, sync=True)  # nobody has moved: no build, the list stays
    assert nl.update_stats() == (2, 1)
    _check(nl, q, BOX10, cull)
    q2 = q.copy()
    q2[:100, 0] = np.clip(q2[:100, 0] + 0.5, 0, np.nextafter(np.float32(BOX10[0]), np.float32(0)))  # past skin / 2
    qd.copy_(torch.from_numpy(q2))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (3, 2)
    _check(nl, q2, BOX10, cull)


@pytest.mark.parametrize("cull", CULL)
def test_one_handle_at_two_sizes(monkeypatch, cull):
    nl = _handle(monkeypatch, cull, 26000, BOX10)
    for n, seed in ((26000, 41), (36000, 42), (26000, 41)):
        q = _uniform(n, seed, BOX10)
        nl.Initialize(n)
        _build(nl, q)
        _check(nl, q, BOX10, cull)


def test_the_plan_leaves_it_out_elsewhere(monkeypatch):
    """No id classes, no cull: a full list, and a sparse box."""
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    q = _uniform(36000, 7, BOX10)
    monkeypatch.delenv("NL_CULL", raising=False)
    nl = NeighListGPU(RC, *BOX10, dtype=torch.float32, full_list=True)
    nl.Initialize(len(q))
    _build(nl, q)
    assert nl.build_info()["id_classes"] == 0 and not nl.build_info()["reach_cull"]
    qs = _uniform(12000, 3, BOX10)
    nl = _handle(monkeypatch, True, len(qs), BOX10)
    _build(nl, qs)
    assert nl.build_info()["small_cells"] and not nl.build_info()["reach_cull"]

"""The expansion's inner loops (k_fill_masks: the walk over the hit bits that puts four rows together in LDS, the row
write-out, the straight-to-memory path of very long rows) at the smallest shapes at which they can go wrong: groups with
dead rows, cells of one, two and three row batches, both states of the high mask plane, rows at the length the LDS copy
holds, empty rows and groups without a single hit, and one box for each of the kernel's other instances.

Every list is compared with the CPU oracle (oracle.pyoracle): counts, key_pointer, every row after the canonical per-row
sort, and nl_list_checksum.  All boxes have at most 5 x 5 x 5 cells.
"""
import numpy as np
import pytest

from tests.test_exclusions import _checksum
from tests.util import canonical_csr

pytestmark = pytest.mark.gpu

RC = 3.3
EDGE = 3.35  # cell edge of the boxes below: int(M * EDGE / RC) = M cells a side for M <= 5
EXPAND_RMAX = {False: 160, True: 192}  # longest row k_fill_masks puts together in LDS (half, full list)


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def _box(m):
    return (m * EDGE,) * 3


def _mesh(box):
    return [int(b / RC) for b in box]


def _cell_of(q, box):
    m = _mesh(box)
    c = [np.minimum((q[:, d].astype(np.float64) / (box[d] / m[d])).astype(np.int64), m[d] - 1) for d in range(3)]
    return c[0] + m[0] * (c[1] + m[1] * c[2])


def _streams(q, box):
    """Stencil-stream length of every cell: the particles of its 27 cells (the stencil wraps, also in an open box)."""
    m = _mesh(box)
    cnt = np.bincount(_cell_of(q, box), minlength=m[0] * m[1] * m[2]).reshape(m[2], m[1], m[0])
    out = np.zeros_like(cnt)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                out += np.roll(cnt, (dz, dy, dx), axis=(0, 1, 2))
    return out.ravel()


def _fill_cells(m, rho, seed, forced=None, dtype=np.float32):
    """A box of m^3 cells: every cell gets a Poisson(rho EDGE^3) number of particles, or forced[(cx, cy, cz)] of them,
    uniformly inside the cell and 0.01 away from its faces (no rounding moves one next door); ids shuffled."""
    rng = np.random.default_rng(seed)
    forced = forced or {}
    pts = []
    for cz in range(m):
        for cy in range(m):
            for cx in range(m):
                k = forced.get((cx, cy, cz), int(rng.poisson(rho * EDGE ** 3)))
                pts.append((np.array([cx, cy, cz]) + rng.uniform(0.01 / EDGE, 1 - 0.01 / EDGE, (k, 3))) * EDGE)
    p = np.concatenate(pts)
    q = np.zeros((len(p), 4), dtype=dtype)
    q[:, :3] = p[rng.permutation(len(p))]
    return q, _box(m)


def _uniform(m, rho, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    box = _box(m)
    n = int(round(rho * box[0] * box[1] * box[2]))
    q = np.zeros((n, 4), dtype=dtype)
    q[:, :3] = rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(box) * (1 - 2.0 ** -20)
    return q, box


def _handle(monkeypatch, q, box, classes=None, full=False, pbc=False, width=None):
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    if classes is not None:
        monkeypatch.setenv("NL_IDCLASS", str(classes))  # (read when the handle is created)
    if width is not None:
        monkeypatch.setenv("NL_OFFSET_WIDTH", str(width))
    nl = NeighListGPU(RC, *box, dtype=torch.float32 if q.dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=pbc)
    nl.Initialize(len(q))
    nl.MakeNeighList(torch.from_numpy(q).cuda(), len(q))
    return nl


def _mirror(ref):
    """(key_pointer, canonical list, counts) of the full list of a canonical half list."""
    n = len(ref.key_pointer) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ref.key_pointer))
    cols = ref.sorted_list.astype(np.int64)
    a, b = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    cnt = np.bincount(a, minlength=n)
    key = np.sort((a << 32) | b)
    return np.concatenate([[0], np.cumsum(cnt)]), (key & 0xFFFFFFFF).astype(np.int32), cnt.astype(np.int32)


def _check(nl, q, box, full=False, pbc=False, wide=False):
    """The handle's list is the oracle's: counts, offsets, every row after the canonical sort, the checksum.  Returns the
    oracle's counts (of the half list, or of the full list)."""
    po = _po()
    ref = (po.build_pbc(q, RC, box) if pbc else po.build(q, RC, box)).canonical()
    if full:
        want_kp, want_lst, want_cnt = _mirror(ref)
        kp, lst, cnt = (t.cpu().numpy() for t in nl.full_csr(64 if wide else 32))
        assert nl.number_of_pairs() == 2 * ref.npairs
    else:
        want_kp, want_lst, want_cnt = ref.key_pointer, ref.sorted_list, ref.number_of_partners
        kp = (nl.key_pointer64() if wide else nl.key_pointer()).cpu().numpy()
        lst, cnt = nl.sorted_list().cpu().numpy(), nl.half_number_of_partners().cpu().numpy()
        assert nl.half_number_of_pairs() == ref.npairs
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(kp.astype(np.int64), want_kp)
    assert np.array_equal(canonical_csr(kp, lst), want_lst)
    assert nl.list_checksum() == (_checksum(want_kp, want_lst), len(want_lst))
    if not full and not pbc:
        assert nl.list_checksum() == (ref.hash(), ref.npairs)
    return want_cnt


def _one_batch_masks(nl, q, box, classes=None, small=0, cap=None):
    """The build expanded hit masks of one LDS batch, and no cell's stream exceeds the batch (it keeps its masks)."""
    info = nl.build_info()
    assert info["masks"] and info["mask_rows"] == 1 and info["fine_rows"] == 0, info
    assert info["small_cells"] == small, info
    if classes is not None:
        assert info["id_classes"] == int(classes), info
    cap = info["lds_batch"] // (2 if small else 1) if cap is None else cap
    assert _streams(q, box).max() <= cap, (_streams(q, box).max(), cap)
    return info


# ------------------------------------------------------------------------------------------ partial groups and batches
# 24 rows a wave and batch, two waves a cell, four rows a group: 1, 2, 3 and 5 particles leave groups with dead rows (and
# a wave without a row), 24 and 25 sit at the edge of a group, 48 is exactly one batch for each wave, 49 and 50 need a
# second batch, 97 a third (49 rows a wave)
CROWDED = {(1, 1, 1): 1, (2, 1, 1): 2, (1, 2, 1): 3, (2, 2, 1): 5, (1, 1, 2): 24, (2, 1, 2): 25, (1, 2, 2): 49,
           (3, 3, 3): 48, (0, 3, 0): 50, (3, 0, 3): 97}


@pytest.mark.parametrize("classes", [0, 2, 4])
def test_partial_groups_and_batches(monkeypatch, classes):
    q, box = _fill_cells(4, 1.0, 21, forced=CROWDED)
    cnt = np.bincount(_cell_of(q, box), minlength=64).reshape(4, 4, 4)
    for (cx, cy, cz), k in CROWDED.items():
        assert cnt[cz, cy, cx] == k
    nl = _handle(monkeypatch, q, box, classes=classes)
    _one_batch_masks(nl, q, box, classes=classes)
    _check(nl, q, box)


# ------------------------------------------------------------------------------------------ both states of the high plane
@pytest.mark.parametrize("classes", [0, 2, 4])
@pytest.mark.parametrize("rho", [0.8, 1.03])
def test_high_plane(monkeypatch, rho, classes):
    """Streams of at most 16 tiles (hit words of 16 bits: the low plane alone) and of 17 and more (both planes)."""
    q, box = _fill_cells(4, rho, 22, forced={(1, 1, 1): 3, (2, 2, 2): 49})
    tiles = (_streams(q, box) + 63) // 64
    if rho < 1:
        assert tiles.max() <= 16, tiles
    else:
        assert (tiles >= 17).sum() >= 16 and (tiles <= 16).sum() >= 8, tiles  # (cells of either kind in one build)
    nl = _handle(monkeypatch, q, box, classes=classes)
    _one_batch_masks(nl, q, box, classes=classes)
    _check(nl, q, box)


# ------------------------------------------------------------------------------------------ row length at the LDS limit
def _blob(k, seed):
    """k particles within RC / 2 of one point (ids 0 .. k - 1: all partners of each other) in a box of 5^3 cells at rho 0.7
    with nothing else within RC of the blob."""
    rng = np.random.default_rng(seed)
    q, box = _uniform(5, 0.7, seed)
    centre = np.array([2.5, 2.5, 2.5]) * EDGE
    far = np.linalg.norm(q[:, :3].astype(np.float64) - centre, axis=1) > 1.5 * RC + 0.1
    v = rng.normal(size=(k, 3))
    v *= (0.5 * RC - 0.01) * rng.uniform(0, 1, (k, 1)) ** (1 / 3) / np.linalg.norm(v, axis=1, keepdims=True)
    out = np.zeros((k + int(far.sum()), 4), dtype=np.float32)
    out[:k, :3] = centre + v
    out[k:] = q[far]
    return out, box


@pytest.mark.parametrize("full,longest", [(False, 159), (False, 160), (False, 161), (True, 191), (True, 192), (True, 193)])
def test_row_length_at_the_lds_limit(monkeypatch, full, longest):
    """The longest row has EXPAND_RMAX - 1, EXPAND_RMAX and EXPAND_RMAX + 1 entries: the last length put together in LDS
    (its free slot is the last of the row's region) and the first two that go straight to memory.  Half list: particle 0
    of the blob has the k - 1 others as partners, particle 1 has k - 2, ...; full list: every one of them has k - 1."""
    assert longest - EXPAND_RMAX[full] in (-1, 0, 1)
    k = longest + 1
    q, box = _blob(k, 23)
    nl = _handle(monkeypatch, q, box, full=full)
    _one_batch_masks(nl, q, box)
    cnt = _check(nl, q, box, full=full)
    assert cnt.max() == longest and cnt[0] == longest
    if full:
        assert (cnt[:k] == longest).all()
    else:
        assert np.array_equal(cnt[:k], np.arange(k - 1, -1, -1))


# ------------------------------------------------------------------------------------------ empty rows
def _with_isolated(seed, cluster=True, lone_at=(0, 3, 7)):
    """A box of 5^3 cells at rho 1 around an emptied region: cell (2, 2, 2) holds three isolated particles in three of its
    corners (nothing within RC of them) and a cluster of five in a fourth corner, 4.6 away from each of the three.  The
    eight have the ids 10 .. 17 (neighbours in the input, so that the binning ranks them the same way in every build);
    lone_at says which of these the three are.  Without the cluster the cell has the three only (ids 10, 11, 12): its
    groups end without a hit.  Returns (q, box, ids of the three, ids of the cell)."""
    rng = np.random.default_rng(seed)
    q, box = _uniform(5, 1.0, seed)
    lo, hi = 2 * EDGE + 0.02, 3 * EDGE - 0.02
    lone = np.array([[lo, lo, lo], [hi, hi, lo], [lo, hi, hi]])
    near = np.array([hi, lo, hi]) + rng.uniform(-0.3, 0.0, (5 if cluster else 0, 3)) * np.array([1, -1, 1])
    p = q[:, :3].astype(np.float64)
    keep = np.ones(len(q), dtype=bool)
    for c in lone:
        keep &= np.linalg.norm(p - c, axis=1) > RC + 0.1
    keep &= _cell_of(q, box) != 2 + 5 * (2 + 5 * 2)
    rest = q[keep]
    n = len(rest) + 3 + len(near)
    out = np.zeros((n, 4), dtype=np.float32)
    cell_ids = list(range(10, 18)) if cluster else [10, 11, 12]
    lone_ids = [cell_ids[k] for k in lone_at] if cluster else cell_ids
    out[lone_ids, :3] = lone
    out[[i for i in cell_ids if i not in lone_ids], :3] = near
    out[np.setdiff1d(np.arange(n), cell_ids)] = rest
    return out, box, lone_ids, cell_ids


@pytest.mark.parametrize("classes,full,cluster", [(0, False, True), (2, False, True), (0, True, True), (2, False, False),
                                                  (0, True, False)])
def test_empty_rows(monkeypatch, classes, full, cluster):
    """Rows without an entry first, in the middle and last in a cell's slot order, one of them the cell's highest id.  The
    slot order of a cell follows from the ids of its particles, not from where in the cell they are: a first build shows
    it, the second build puts the three isolated particles on the ids of the first, a middle and the last slot."""
    q, box, lone, cell_ids = _with_isolated(24, cluster)

    def slots(nl):
        order = nl.cell_order().cpu().numpy()
        return [int(i) for i in order[np.isin(order, cell_ids)]]

    want = [0, 1, 2]
    if cluster:
        first = slots(_handle(monkeypatch, q, box, classes=classes, full=full))
        assert sorted(first) == cell_ids
        top = first.index(cell_ids[-1])
        want = [0, top if 0 < top < 7 else 3, 7]
        q, box, lone, _ = _with_isolated(24, True, lone_at=[cell_ids.index(first[s]) for s in want])
    nl = _handle(monkeypatch, q, box, classes=classes, full=full)
    _one_batch_masks(nl, q, box, classes=None if full else classes)
    cnt = _check(nl, q, box, full=full)
    assert (cnt[lone] == 0).all()
    assert sorted(slots(nl).index(i) for i in lone) == want, slots(nl)
    assert cell_ids[-1] in lone


def test_cells_of_empty_rows_only(monkeypatch):
    """Particles on a lattice wider than the cut-off, several to a cell: no row has an entry, every group of four rows
    ends without a hit."""
    m = 5
    g = np.stack(np.meshgrid(*(np.arange(7),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # spacing 2.39: sqrt(2) 2.39 > RC
    g = g[g.sum(axis=1) % 2 == 0]  # (fcc-like: nearest neighbours at 3.38)
    q = np.zeros((len(g), 4), dtype=np.float32)
    q[:, :3] = 0.05 + g * (m * EDGE - 0.1) / 7
    q = q[np.random.default_rng(25).permutation(len(q))]
    for full in (False, True):
        nl = _handle(monkeypatch, q, _box(m), classes=0, full=full)
        assert nl.build_info()["masks"]
        cnt = _check(nl, q, _box(m), full=full)
        assert cnt.sum() == 0


# ------------------------------------------------------------------------------------------ the other instances
def test_sparse_box_one_wave_per_cell(monkeypatch):
    """rho 0.5: the one-wave instance with the ids of half a stream."""
    q, box = _uniform(5, 0.5, 26)
    for full in (False, True):
        nl = _handle(monkeypatch, q, box, full=full)
        _one_batch_masks(nl, q, box, small=1)
        _check(nl, q, box, full=full)


@pytest.mark.parametrize("classes", [0, 2, 4])
def test_twelve_rows_a_batch(monkeypatch, classes):
    """20.3 particles a cell: too many for the one-wave instance, few enough for the instances that load 12 rows a
    batch (cells of more than 24 particles take a second batch there)."""
    q, box = _uniform(5, 0.54, 27)
    assert 19.7 * 125 < len(q) <= 21 * 125 and np.bincount(_cell_of(q, box)).max() > 24
    nl = _handle(monkeypatch, q, box, classes=classes)
    _one_batch_masks(nl, q, box, classes=classes)
    _check(nl, q, box)


@pytest.mark.parametrize("rho", [0.54, 1.0])
def test_full_list(monkeypatch, rho):
    q, box = _uniform(5, rho, 28)
    nl = _handle(monkeypatch, q, box, full=True)
    _one_batch_masks(nl, q, box)
    _check(nl, q, box, full=True)


@pytest.mark.parametrize("full", [False, True])
def test_periodic_axes(monkeypatch, full):
    q, box = _uniform(5, 1.0, 29)
    nl = _handle(monkeypatch, q, box, full=full, pbc=True)
    _one_batch_masks(nl, q, box)
    _check(nl, q, box, full=full, pbc=True)


@pytest.mark.parametrize("full", [False, True])
def test_wide_offsets(monkeypatch, full):
    q, box = _uniform(5, 1.0, 30)
    nl = _handle(monkeypatch, q, box, full=full, width=64)
    assert _one_batch_masks(nl, q, box)["offset_bits"] == 64
    _check(nl, q, box, full=full, wide=True)


@pytest.mark.parametrize("full", [False, True])
def test_fp64_positions(monkeypatch, full):
    """fp64 at rho 0.5: every stream fits the (smaller) fp64 batch."""
    q, box = _uniform(5, 0.5, 31, dtype=np.float64)
    nl = _handle(monkeypatch, q, box, full=full)
    _one_batch_masks(nl, q, box)
    _check(nl, q, box, full=full)

"""Triclinic boxes and box changes between builds (nl_set_box): binning in sheared coordinates, images at lattice vectors.

The C oracle has no tilt, so the reference here is `replay`: the rule of include/nl_hip.h (nl_set_box) in numpy, in exact
position-type arithmetic (float32 / float64 operations, no FMA).  It is anchored in two directions on the CPU:
  * against an independent float64 brute force, the minimum distance over the 27 lattice images, which may differ from
    it only in a band around the cut-off sized to the rounding of the position type;
  * at zero tilt, bit for bit against pyoracle.build (mask 0) and pyoracle.build_pbc (mask 7).
Every GPU list is compared with the replay after the canonical sort, bit for bit.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.util import canonical_csr, check_lj, lj_list_separations, lj_pair_magnitudes, lj_rows_off_the_band

CFG2_L = 101.594  # BASELINE config 2 box
RC = 3.3


def _torch():
    import torch

    return torch


def _po():
    from oracle import pyoracle as po

    return po


# ------------------------------------------------------------------------------------------------------ the rule
def floor_to(v, T):
    f = T(v)
    if float(f) > v:
        f = np.nextafter(f, T(-np.inf))
    return f


def rc2_of(rc, T):
    return floor_to(rc * rc, T) if T == np.float32 else T(rc * rc)


def mesh_of(rc, box):
    """m_d = (int)(w_d / rc) from the perpendicular widths (nl_hip.h, nl_set_box)."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    sx = (xy * yz - Ly * xz) / (Ly * Lz)
    w = (Lx / np.sqrt(1.0 + (xy / Ly) * (xy / Ly) + sx * sx), Ly / np.sqrt(1.0 + (yz / Lz) * (yz / Lz)), Lz)
    return tuple(int(v / rc) for v in w)


def shear_of(box, T):
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    return T(xy / Ly), T((xz * Ly - xy * yz) / (Ly * Lz)), T(yz / Lz)


def lattice(box, n):
    """S(n) = n_a a + n_b b + n_c c in float64 (n: [k, 3] ints), the order of lattice_shift."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    n = np.asarray(n, dtype=np.float64)
    sx = (n[:, 0] * Lx + n[:, 1] * xy) + n[:, 2] * xz
    sy = n[:, 1] * Ly + n[:, 2] * yz
    sz = n[:, 2] * Lz
    return np.stack([sx, sy, sz], axis=1)


def bin_frame(q, rc, box, mask, T):
    """(stored positions, cell index per axis, out-of-box flag): local_cell of nl_kernels.hpp with the tilt, in numpy."""
    x = q[:, :3].astype(T)
    m = mesh_of(rc, box)
    kxy, kxz, kyz = shear_of(box, T)
    tilt = any(float(v) != 0.0 for v in box[3:])
    xs, ys = x[:, 0], x[:, 1]
    if tilt:
        xs = (x[:, 0] - x[:, 1] * kxy) - x[:, 2] * kxz
        ys = x[:, 1] - x[:, 2] * kyz
    sheared = (xs, ys, x[:, 2])
    cells = np.zeros((len(q), 3), dtype=np.int64)
    wrap = np.zeros((len(q), 3), dtype=np.int64)
    bad = np.zeros(len(q), dtype=bool)
    for d in range(3):
        ms = float(box[d]) / m[d]
        ims = T(1.0 / float(np.float32(ms))) if T == np.float32 else T(1.0 / ms)
        t = sheared[d] * ims
        bad |= ~((t > T(-2147483000.0)) & (t < T(2147483000.0)))
        t = np.where(bad, T(0), t)
        v = np.trunc(t).astype(np.int64)
        per = bool(mask >> d & 1)
        if per:
            v -= ((t < 0) & (v.astype(T) != t)).astype(np.int64)
        lo, hi = v < 0, v >= m[d]
        v = np.where(lo, v + m[d], np.where(hi, v - m[d], v))
        if per:
            wrap[:, d] = np.where(lo, 1, np.where(hi, -1, 0))
        bad |= (v < 0) | (v >= m[d])
        cells[:, d] = v
    out = x.copy()
    if tilt:
        S = lattice(box, wrap).astype(T)
    else:
        S = np.zeros_like(x)
        for d in range(3):
            S[:, d] = wrap[:, d].astype(T) * T(box[d])
    for d in range(3):
        if mask >> d & 1:
            out[:, d] = out[:, d] + S[:, d]
    return out, cells, bad


def replay_pairs(q, rc, box, mask, T, full=False):
    """The list of the rule: (rows, partners) of every entry, decided as the search decides it (27-cell stencil over
    sheared cells, partner staged at q_stored + S(w), r2 = (dx^2 + dy^2) + dz^2 in T, kept unless r2 > rc2)."""
    box = tuple(float(v) for v in box) + (0.0,) * (6 - len(box))
    pos, cells, bad = bin_frame(q, rc, box, mask, T)
    assert not bad.any(), "replay: a particle outside the box"
    m = mesh_of(rc, box)
    n = len(q)
    cid = cells[:, 0] + m[0] * (cells[:, 1] + m[1] * cells[:, 2])
    order = np.argsort(cid, kind="stable")
    ncell = m[0] * m[1] * m[2]
    start = np.zeros(ncell + 1, dtype=np.int64)
    np.add.at(start, cid + 1, 1)
    start = np.cumsum(start)
    rc2 = rc2_of(rc, T)
    rows, parts = [], []
    for o in itertools.product((-1, 0, 1), repeat=3):
        nc = cells + np.array(o)
        w = np.zeros_like(nc)
        for d in range(3):
            lo, hi = nc[:, d] < 0, nc[:, d] >= m[d]
            nc[:, d] = np.where(lo, nc[:, d] + m[d], np.where(hi, nc[:, d] - m[d], nc[:, d]))
            if mask >> d & 1:
                w[:, d] = np.where(lo, -1, np.where(hi, 1, 0))
        c2 = nc[:, 0] + m[0] * (nc[:, 1] + m[1] * nc[:, 2])
        cnt = start[c2 + 1] - start[c2]
        i = np.repeat(np.arange(n), cnt)
        base = np.repeat(start[c2] - np.cumsum(cnt) + cnt, cnt)
        j = order[base + np.arange(cnt.sum())]
        keep = (j != i) if full else (j > i)
        i, j = i[keep], j[keep]
        wi = w[i]
        S = lattice(box, wi).astype(T) if any(box[3:]) else wi.astype(T) * np.array(box[:3], dtype=T)
        d2 = []
        for d in range(3):
            pj = pos[j, d] + S[:, d] if mask >> d & 1 else pos[j, d]
            d2.append(pj - pos[i, d])
        r2 = (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2]
        ok = ~(r2 > rc2)
        rows.append(i[ok])
        parts.append(j[ok])
    return np.concatenate(rows), np.concatenate(parts), n


def to_csr(rows, parts, n):
    order = np.lexsort((parts, rows))
    kp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(kp, rows + 1, 1)
    return np.cumsum(kp), parts[order].astype(np.int32)


def replay(q, rc, box, mask, T, full=False):
    return to_csr(*replay_pairs(q, rc, box, mask, T, full))


def search_r2(q, rc, box, mask, T, rows, parts):
    """r2 of entries (row, partner) as the search tests them: both at their stored images, the partner shifted by S(w) of
    the faces through which the row's stencil reaches its cell."""
    box = tuple(float(v) for v in box) + (0.0,) * (6 - len(box))
    pos, cells, _ = bin_frame(q, rc, box, mask, T)
    m = mesh_of(rc, box)
    w = np.zeros((len(rows), 3), dtype=np.int64)
    for d in range(3):
        if mask >> d & 1:
            ci, cj = cells[rows, d], cells[parts, d]
            w[:, d] = np.where((ci == 0) & (cj == m[d] - 1), -1, np.where((ci == m[d] - 1) & (cj == 0), 1, 0))
    S = lattice(box, w).astype(T)
    dd = [(pos[parts, d] + S[:, d] if mask >> d & 1 else pos[parts, d]) - pos[rows, d] for d in range(3)]
    return (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]


def brute_force(q, rc, box, mask):
    """float64: pairs (i < j) whose minimum distance over the lattice images of the periodic axes is <= rc, and the pairs
    within a relative 1e-5 of the cut-off (left undecided)."""
    p = q[:, :3].astype(np.float64)
    box = tuple(float(v) for v in box)
    ns = [n for n in itertools.product((-1, 0, 1), repeat=3) if all(n[d] == 0 or mask >> d & 1 for d in range(3))]
    S = lattice(box, np.array(ns))
    best = None
    for s in S:
        d = p[None, :, :] + s[None, None, :] - p[:, None, :]
        r2 = (d * d).sum(axis=2)
        best = r2 if best is None else np.minimum(best, r2)
    iu = np.triu_indices(len(p), 1)
    r2 = best[iu]
    keep = set(zip(iu[0][r2 <= rc * rc].tolist(), iu[1][r2 <= rc * rc].tolist()))
    band = np.abs(np.sqrt(r2) - rc) <= 1e-5 * rc
    edge = set(zip(iu[0][band].tolist(), iu[1][band].tolist()))
    return keep, edge


def positions(n, rc, box, mask, T, seed, above_open=True):
    """Uniform in the cell coordinates lambda, plus particles at lambda = 0, just below 1, slightly negative and
    slightly above 1 on every periodic axis; on an open axis up to rc/2 above the box."""
    box = tuple(float(v) for v in box) + (0.0,) * (6 - len(box))
    rng = np.random.default_rng(seed)
    lam = rng.uniform(0.0, 1.0, size=(n, 3))
    k = max(n // 80, 4)
    for d in range(3):
        idx = rng.choice(n, 4 * k, replace=False)
        if mask >> d & 1:
            lam[idx[:k], d] = 0.0
            lam[idx[k:2 * k], d] = 1.0 - 1e-7
            lam[idx[2 * k:3 * k], d] = -rng.uniform(0.0, 0.1, size=k)
            lam[idx[3 * k:], d] = 1.0 + rng.uniform(0.0, 0.1, size=k)
        elif above_open:
            lam[idx[:k], d] = 1.0 + rng.uniform(0.0, 0.49 * rc / float(box[d]), size=k)
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    p = np.stack([lam[:, 0] * Lx + lam[:, 1] * xy + lam[:, 2] * xz, lam[:, 1] * Ly + lam[:, 2] * yz, lam[:, 2] * Lz], axis=1)
    q = np.zeros((n, 4), dtype=T)
    q[:, :3] = p.astype(T)
    return q


# Edges and tilts that float32 cannot hold, nor their sums: S(w) rounded twice (a, b, c to T first) differs from the rule
BOX = (27.3, 24.1, 30.7)
TILTS = {
    "xy": (0.2 * 27.3, 0.0, 0.0),
    "all": (0.2 * 27.3, -0.15 * 27.3, 0.23 * 24.1),
    "neg": (-0.26 * 27.3, 0.0, 0.0),
    "half": (0.5 * 27.3, 0.5 * 27.3, 0.5 * 24.1),
}


def tilted(tilt_name, mask):
    t = TILTS[tilt_name]
    if mask == 3:
        t = (t[0], 0.0, 0.0)
    return BOX + t


# ------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [7, 3])
@pytest.mark.parametrize("tilt", sorted(TILTS))
def test_replay_equals_brute_force_up_to_rounding(dtype, mask, tilt):
    box = tilted(tilt, mask)
    q = positions(900, RC, box, mask, dtype, seed=11)
    rows, parts, n = replay_pairs(q, RC, box, mask, dtype)
    got = set(zip(rows.tolist(), parts.tolist()))
    assert len(got) == len(rows), "a pair listed twice"
    keep, edge = brute_force(q, RC, box, mask)
    assert got - edge == keep - edge
    assert len(keep) > 1000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [0, 7])
def test_replay_at_zero_tilt_is_the_oracle(dtype, mask):
    po = _po()
    rng = np.random.default_rng(5)
    n = 3000
    q = np.zeros((n, 4), dtype=dtype)
    q[:, :3] = (rng.uniform(0.0, 1.0, size=(n, 3)) * np.array(BOX)).astype(dtype)
    q[:40, 0] = dtype(0.0)
    q[40:80, 1] = dtype(BOX[1]) - dtype(1e-5)
    ref = po.build(q, RC, BOX) if mask == 0 else po.build_pbc(q, RC, BOX)
    kp, sl = replay(q, RC, BOX + (0.0, 0.0, 0.0), mask, dtype)
    refc = ref.canonical()
    assert np.array_equal(kp, refc.key_pointer)
    assert np.array_equal(sl, refc.sorted_list)


def test_mesh_of_the_cfg2_box():
    L = CFG2_L
    assert mesh_of(RC, (L, L, L, 0.2 * L, 0.0, 0.0)) == (30, 30, 30)
    assert mesh_of(RC, (L, L, L, 0.5 * L, 0.0, 0.0)) == (27, 30, 30)
    assert mesh_of(RC, (L, L, L, 0.5 * L, 0.5 * L, 0.5 * L)) == (26, 27, 30)
    assert mesh_of(RC, (L, L, L, 0.0, 0.0, 0.0)) == tuple(int(L / RC) for _ in range(3))


# ------------------------------------------------------------------------------------------------------- GPU tests
def _handle(box, dtype, mask, n, full=False, **kw):
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    nl = NeighListGPU(RC if "rc" not in kw else kw["rc"], box[0], box[1], box[2],
                      dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image={0: False, 7: True}.get(mask, "".join("xyz"[d] for d in range(3) if mask >> d & 1)),
                      tilt=box[3:6] if len(box) > 3 else None)
    nl.Initialize(n)
    return nl


def _csr(nl, full=False):
    if full:
        kp, lst, _cnt = nl.full_csr(64)
        kp = kp.cpu().numpy()
        return kp, canonical_csr(kp, lst.cpu().numpy())
    kp = nl.key_pointer64().cpu().numpy()
    return kp, canonical_csr(kp, nl.sorted_list().cpu().numpy())


def _check(nl, q, box, mask, dtype, full=False, rc=RC):
    kp, sl = _csr(nl, full)
    rkp, rsl = replay(q, rc, box, mask, dtype, full)
    assert np.array_equal(kp, rkp)
    assert np.array_equal(sl, rsl)
    return len(rsl)


def _build(nl, q, sync=True):
    torch = _torch()
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(qd, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return qd


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask,tilt", [(7, "xy"), (7, "all"), (7, "neg"), (7, "half"), (3, "xy"), (3, "half")])
@pytest.mark.parametrize("full", [False, True])
def test_tilted_list_equals_replay(dtype, mask, tilt, full):
    box = tilted(tilt, mask)
    q = positions(20000, RC, box, mask, dtype, seed=3)
    nl = _handle(box, dtype, mask, len(q), full=full)
    _build(nl, q)
    assert nl.mesh_size == mesh_of(RC, box)
    assert _check(nl, q, box, mask, dtype, full) > 100000


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"NL_SWEEP_VARIANT": "1"}, {"NL_BINNING": "1"}, {"NL_BIN_BUCKETS": "0"},
                                 {"NL_OFFSET_WIDTH": "32"}, {"NL_OFFSET_WIDTH": "64"}])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tilted_paths(env, dtype, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    box = tilted("all", 7)
    q = positions(20000, RC, box, 7, dtype, seed=4)
    nl = _handle(box, dtype, 7, len(q))
    _build(nl, q)
    _check(nl, q, box, 7, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tilted_dense_and_screened(dtype):
    # about 90 particles a cell: hit masks per LDS batch + k_fill_dense; fp64 runs the screened search there
    box = (24.3, 24.1, 23.9, 7.1, -5.2, 4.3)
    rc = 4.0
    m = mesh_of(rc, box)
    n = 90 * m[0] * m[1] * m[2]
    q = positions(n, rc, box, 7, dtype, seed=8)
    nl = _handle(box, dtype, 7, n, rc=rc)
    _build(nl, q)
    assert nl.build_info()["mask_rows"] > 1 or dtype == np.float64
    _check(nl, q, box, 7, dtype, rc=rc)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cutoff_band_across_tilted_faces(dtype):
    """Pairs that the replay puts within a few ulp of rc^2, on both sides, through faces and edges: the partner is
    placed at rc (1 + e) from its row particle along directions that cross the tilted faces."""
    box = tilted("all", 7)
    rng = np.random.default_rng(21)
    base = positions(4000, RC, box, 7, dtype, seed=22)
    a, b, c = np.array([box[0], 0, 0]), np.array([box[3], box[1], 0]), np.array([box[4], box[5], box[2]])
    extra = []
    for corner in itertools.product((0.0, 1.0 - 1e-6), repeat=3):
        p0 = corner[0] * a + corner[1] * b + corner[2] * c
        for _ in range(12):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            for e in (-4e-7, -1e-7, 0.0, 1e-7, 4e-7) if dtype == np.float32 else (-1e-15, -3e-16, 0.0, 3e-16, 1e-15):
                extra.append(p0)
                extra.append(p0 + RC * (1.0 + e) * u)
    ex = np.zeros((len(extra), 4), dtype=dtype)
    ex[:, :3] = np.array(extra).astype(dtype)
    q = np.concatenate([base, ex])
    # the constructed pairs lie within a few ulp of rc2 on both sides, through the faces and edges of the tilted cell
    i = len(base) + 2 * np.arange(len(extra) // 2)
    r2 = search_r2(q, RC, box, 7, dtype, i, i + 1)
    rc2 = rc2_of(RC, dtype)
    ulp = np.spacing(rc2)
    near = np.abs(r2 - rc2) <= 32 * ulp
    assert (near & (r2 <= rc2)).sum() >= 10 and (near & (r2 > rc2)).sum() >= 10
    nl = _handle(box, dtype, 7, len(q))
    _build(nl, q)
    _check(nl, q, box, 7, dtype)
    nl.set_full_list(True)
    _build(nl, q)
    _check(nl, q, box, 7, dtype, full=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_set_box_with_creation_box_changes_nothing(dtype):
    q = positions(12000, RC, BOX + (0, 0, 0), 7, dtype, seed=9, above_open=False)
    for mask in range(8):
        a = _handle(BOX, dtype, mask, len(q))
        b = _handle(BOX, dtype, mask, len(q))
        b.set_box(*BOX)
        b.set_box(*BOX, 0.0, 0.0, 0.0)
        _build(a, q)
        _build(b, q)
        assert a.list_checksum() == b.list_checksum()
        assert all(np.array_equal(x, y) for x, y in zip(_csr(a), _csr(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_changes_equal_a_fresh_handle(dtype):
    nl = _handle(BOX, dtype, 7, 30000)
    for box in [(40.3, 36.1, 33.7, 8.1, 3.3, -2.2), (14.1, 12.3, 13.4, 2.1, 0.0, 1.3), BOX + (0.0, 0.0, 0.0),
                BOX + (0.5 * BOX[0], 0.0, 0.0)]:
        nl.set_box(*box)
        assert nl.box == tuple(float(v) for v in box)
        assert nl.mesh_size == mesh_of(RC, box)
        q = positions(30000 if box[0] > 20 else 4000, RC, box, 7, dtype, seed=int(box[0]))
        nl.set_capacity(1000)  # (a synchronous build still grows its list)
        _build(nl, q)
        n = _check(nl, q, box, 7, dtype)
        fresh = _handle(box, dtype, 7, len(q))
        _build(fresh, q)
        assert fresh.list_checksum() == nl.list_checksum()
        assert n > 0


@pytest.mark.gpu
def test_exclusions_and_type_cutoffs_with_tilt():
    torch = _torch()
    dtype = np.float32
    box = tilted("all", 7)
    q = positions(15000, RC, box, 7, dtype, seed=31)
    rows, parts, n = replay_pairs(q, RC, box, 7, dtype)
    rng = np.random.default_rng(2)
    types = rng.integers(0, 2, size=n).astype(np.int32)
    rcm = np.array([[3.3, 2.5], [2.5, 1.8]])
    # type rule: keep iff !(r2 > rc2[t_i][t_j]), r2 at the image the search used
    r2 = search_r2(q, RC, box, 7, dtype, rows, parts)
    thr = np.array([[floor_to(r * r, dtype) for r in row] for row in rcm], dtype=dtype)
    keep = ~(r2 > thr[types[rows], types[parts]])
    excl = np.stack([rows[::7], parts[::7]], axis=1).astype(np.int32)
    keep &= ~np.isin(rows.astype(np.int64) * n + parts, excl[:, 0].astype(np.int64) * n + excl[:, 1])
    ekp, esl = to_csr(rows[keep], parts[keep], n)
    nl = _handle(box, dtype, 7, n)
    nl.set_exclusions(torch.from_numpy(excl).cuda(), n)
    nl.set_type_cutoffs(torch.from_numpy(types).cuda(), rcm)
    _build(nl, q)
    kp, sl = _csr(nl)
    assert np.array_equal(kp, ekp) and np.array_equal(sl, esl)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_list_with_tilt(dtype):
    torch = _torch()
    box = tilted("all", 7)
    q = positions(20000, RC, box, 7, dtype, seed=41)
    nl = _handle(box, dtype, 7, len(q))
    skin = 0.4
    nl.set_skin(skin)
    qd = torch.from_numpy(q.copy()).cuda()
    nl.update(qd, len(q), sync=True)
    assert nl.update_stats() == (1, 1)
    # small moves, and particles re-wrapped by the caller through a tilted face (q - c)
    rng = np.random.default_rng(1)
    q2 = q.copy()
    q2[:, :3] += (rng.uniform(-1, 1, size=(len(q), 3)) * 0.1 * skin / np.sqrt(3)).astype(dtype)
    c = np.array([box[4], box[5], box[2]])
    moved = np.argsort(q[:, 2])[-50:]
    q2[moved, :3] = (q2[moved, :3].astype(np.float64) - c).astype(dtype)
    qd.copy_(torch.from_numpy(q2))
    nl.update(qd, len(q), sync=True)
    assert nl.update_stats() == (2, 1)
    # a move above skin / 2
    q3 = q2.copy()
    q3[5, 0] += dtype(0.3)
    qd.copy_(torch.from_numpy(q3))
    nl.update(qd, len(q), sync=True)
    assert nl.update_stats() == (3, 2)
    _check(nl, q3, box, 7, dtype)
    nl.set_box(*box)  # the same box: no build
    nl.update(qd, len(q), sync=True)
    assert nl.update_stats() == (4, 2)
    box2 = box[:3] + (box[3] + 0.5, box[4], box[5])
    nl.set_box(*box2)  # a changed box: a build
    nl.update(qd, len(q), sync=True)
    assert nl.update_stats() == (5, 3)
    _check(nl, q3, box2, 7, dtype)


@pytest.mark.gpu
def test_graph_replay_across_set_box_and_resort():
    torch = _torch()
    dtype = np.float32
    box = tilted("xy", 7)
    q = positions(20000, RC, box, 7, dtype, seed=51)
    nl = _handle(box, dtype, 7, len(q))
    nl.set_graph(True)
    qd = _build(nl, q, sync=False)
    _check(nl, q, box, 7, dtype)
    box2 = tilted("all", 7)
    nl.set_box(*box2)
    q2 = positions(20000, RC, box2, 7, dtype, seed=52)
    qd.copy_(torch.from_numpy(q2))
    nl.MakeNeighList(qd, len(q2), sync=False)
    nl.synchronize()
    _check(nl, q2, box2, 7, dtype)
    nl.resort(qd)
    nl.MakeNeighList(qd, len(q2), sync=False)
    nl.synchronize()
    _check(nl, qd.cpu().numpy(), box2, 7, dtype)


def _lj_reference(q, rows, parts, box, eps, sig, rcf, with_bound=False):
    d = lj_list_separations(q, rows, parts, box, 7)  # (z, y, x order with the tilts; folded before it is rounded to float64)
    r2 = (d * d).sum(axis=1)
    inn = (r2 < rcf * rcf) & (r2 > 0)
    ir2 = np.where(inn, sig * sig / r2, 0.0)
    s6 = ir2 ** 3
    fr = np.where(inn, 24.0 * eps * (2.0 * s6 - 1.0) * s6 / r2, 0.0)
    pe = np.where(inn, 4.0 * eps * (s6 - 1.0) * s6, 0.0)
    f = np.zeros((len(q), 4))
    for c in range(3):
        np.add.at(f[:, c], rows, fr * d[:, c])
        np.add.at(f[:, c], parts, -fr * d[:, c])
    np.add.at(f[:, 3], rows, 0.5 * pe)
    np.add.at(f[:, 3], parts, 0.5 * pe)
    if with_bound:  # (S of check_lj, and the particles off the 64-ulp band of rc_force)
        ok = inn | (r2 >= rcf * rcf)
        S = lj_pair_magnitudes(len(q), rows[ok], parts[ok], d[ok], r2[ok], eps, sig, inn[ok])
        return f, S, lj_rows_off_the_band(len(q), rows[ok], parts[ok], r2[ok], rcf, q.dtype)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
def test_lj_forces_triclinic(dtype, full):
    """Forces in a box with large tilts against float64 numpy over the replayed list, scalar and typed.  The box is not
    representable in float32 and the library works with the box in the position type (the binning, the list and the
    consumer's fold alike), so the reference folds with the box rounded to dtype: L differs from (float)L by up to 16 u of
    a separation near 1, which across a face is far beyond c u S for the unthinned close pairs of this input."""
    torch = _torch()
    box = (20.3, 18.1, 19.4, 9.1, -6.2, 8.3)  # large tilts: the single half-box test would miss images
    q = positions(6000, RC, box, 7, np.float64, seed=61).astype(dtype)
    nl = _handle(box, dtype, 7, len(q), full=full)
    qd = _build(nl, q)
    rows, parts, _ = replay_pairs(q, RC, box, 7, dtype)
    ref, S, off_band = _lj_reference(q, rows, parts, tuple(float(dtype(v)) for v in box), 1.0, 1.0, 2.5, with_bound=True)
    f = nl.lj_forces(qd, epsilon=1.0, sigma=1.0, rc_force=2.5).cpu().numpy().astype(np.float64)
    tol = 2e-3 if dtype == np.float32 else 1e-9
    assert np.allclose(f, ref, rtol=tol, atol=tol * (1.0 + np.abs(ref).max()))
    check_lj(f, ref, S, dtype, rows=off_band)  # per particle and component within c u S (tests/test_lj_consumer.py)
    types = np.zeros(len(q), dtype=np.int32)
    types[::3] = 1
    nl.set_type_cutoffs(torch.from_numpy(types).cuda(), np.full((2, 2), RC))
    _build(nl, q)
    nl.set_lj_type_params(np.ones((2, 2)), np.ones((2, 2)), np.full((2, 2), 2.5))
    ft = nl.lj_forces_typed(qd).cpu().numpy().astype(np.float64)
    assert np.allclose(ft, ref, rtol=tol, atol=tol * (1.0 + np.abs(ref).max()))
    check_lj(ft, ref, S, dtype, rows=off_band)


@pytest.mark.gpu
def test_errors_leave_the_box():
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd._lib import NLError

    NL_ERR_ARG, NL_ERR_OUT_OF_BOX, NL_ERR_STATE, NL_ERR_MESH = 1, 3, 6, 7
    torch = _torch()
    dtype = np.float32
    nl = _handle(BOX, dtype, 3, 5000)
    lib, h = nl._lib, nl._h
    q = positions(5000, RC, BOX, 3, dtype, seed=1)
    for tilt in ((0.0, 2.0, 0.0), (0.0, 0.0, 3.0)):  # xz, yz with z open: the box is taken, the build refused
        nl.set_box(*BOX, *tilt)
        assert nl.box == BOX + tilt
        with pytest.raises(NLError) as e:
            _build(nl, q)
        assert e.value.code == NL_ERR_STATE
    nl.set_box(*BOX, 4.0, 0.0, 0.0)  # the hexagonal slab: allowed
    _build(nl, positions(5000, RC, BOX + (4.0, 0.0, 0.0), 3, dtype, seed=2))
    before = nl.box
    for bad, code in [((float("nan"), 24.0, 30.0, 0, 0, 0), NL_ERR_ARG), ((27.0, 0.0, 30.0, 0, 0, 0), NL_ERR_ARG),
                      ((27.0, 24.0, 30.0, float("inf"), 0, 0), NL_ERR_ARG), ((27.0, 24.0, 9.0, 0, 0, 0), NL_ERR_MESH),
                      ((27.0, 24.0, 30.0, 0.0, 0.0, 100.0), NL_ERR_MESH)]:
        assert lib.nl_set_box(h, *[C.c_double(v) for v in bad]) == code
        assert nl.box == before
        assert nl.mesh_size == mesh_of(RC, before)
    # a particle inside [0, L)^3 in Cartesian coordinates but more than a box length outside in sheared ones:
    # x' = x - y xy / Ly = 1 - 23.9 * 40 / 24.1 < -Lx
    big = BOX + (40.0, 0.0, 0.0)
    nl.set_box(*big)
    qb = positions(5000, RC, big, 3, dtype, seed=3)
    qb[7, :3] = np.array([1.0, 23.9, 5.0], dtype=dtype)
    assert (qb[7, :3] >= 0).all() and (qb[7, :3] < np.array(BOX, dtype=dtype)).all()
    with pytest.raises(NLError) as e:
        _build(nl, qb)
    assert e.value.code == NL_ERR_OUT_OF_BOX
    # slab and distributed builds after a change
    nl2 = _handle(BOX, dtype, 7, 5000)
    nl2.set_box(28.0, 24.0, 30.0)
    q2 = positions(5000, RC, (28.0, 24.0, 30.0), 7, dtype, seed=4)
    qd = torch.from_numpy(q2).cuda()
    gid = torch.arange(len(q2), dtype=torch.int32, device="cuda")
    with pytest.raises(NLError) as e:
        nl2.MakeNeighListSlab(qd, gid, len(q2), 0, nl2.mesh_size[2])
    assert e.value.code == NL_ERR_STATE
    cb = _lib.SENDRECV_FN(lambda *args: 0)
    comm = C.c_void_p()
    assert lib.nl_comm_create_callbacks(C.byref(comm), 0, 1, cb, None, torch.cuda.current_device()) == 0
    try:
        assert lib.nl_make_list_distributed(nl2._h, comm, C.c_void_p(qd.data_ptr()), len(q2), len(q2), None, 1) == NL_ERR_STATE
    finally:
        lib.nl_comm_destroy(comm)


@pytest.mark.gpu
def test_set_box_on_a_handle_initialised_for_no_particles():
    """nl_initialize(h, 0) allocates the mesh buffers: a box with more cells regrows them before an empty build."""
    torch = _torch()
    nl = _handle((12.0, 12.0, 12.0), np.float32, 7, 0)
    box = (40.3, 36.1, 33.7, 8.1, 3.3, -2.2)
    nl.set_box(*box)
    assert nl.mesh_size == mesh_of(RC, box)
    nl.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    assert nl.half_number_of_pairs() == 0 and nl.key_pointer().cpu().tolist() == [0]
    q = positions(20000, RC, box, 7, np.float32, seed=71)
    nl.Initialize(len(q))
    _build(nl, q)
    assert _check(nl, q, box, 7, np.float32) > 0


@pytest.mark.gpu
def test_python_surface():
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    nl = NeighListGPU(RC, 27.0, 24.0, 30.0, dtype=torch.float32, minimum_image=True, tilt=(3.0, 1.0, -2.0))
    assert nl.box == (27.0, 24.0, 30.0, 3.0, 1.0, -2.0)
    nl.set_box(30.0, 24.0, 30.0)
    assert nl.box == (30.0, 24.0, 30.0, 0.0, 0.0, 0.0)
    assert nl.mesh_size == (9, 7, 9)

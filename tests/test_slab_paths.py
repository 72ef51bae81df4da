"""Slab builds (nl_make_list_slab) on every search path, list kind and id form, row by row against the oracle.

Row r of a slab build must equal row gid[r] of the list of the undivided box, so every comparison here is exact: the
expected rows are cut out of the oracle's global list (oracle.build, build_pbc, the symmetrised list, build_pbc_full, the
padded reference of tests/test_periodic_axes.py for mixed masks), never out of a second run of the library.  One process:
the slabs of a decomposition are built one after another on one device.  Every case asserts through build_info() /
build_stats() that the path it is meant to cover was the one taken.

Boxes (rc = 3.3): A = 3 x 3 x 7 cells (every cell at the periodic wrap in x and y), B = 5 x 4 x 6 (mx != my), C = 5 x 5 x 8
(room for a low mean density around a crowd).  Densities in particles per cell of the global mesh, which the slabs keep:
8 (mean stencil stream 216: the small instances), 30 (815: one-batch masks), 50 (1360: fine rows in fp32 with an open box,
else two mask rows), 90 (2430: three mask rows).  The thresholds are plan_build's (nl_api.hip).
"""
import functools

import numpy as np
import pytest

from md_neighbor_list_amd import inputs, slab
from tests.test_periodic_axes import reference as padded_reference

RC = 3.3
BOXES = {"A": (10.5, 10.5, 24.0), "B": (17.0, 13.5, 20.5), "C": (17.0, 17.0, 27.5),
         "D": (10.5, 10.5, 10.5), "E": (10.5, 10.5, 13.5)}  # D = 3 x 3 x 3, E = 3 x 3 x 4: tests/test_distributed_paths.py
DECOMPS = {
    "A1": ("A", ((0, 1), (1, 4), (4, 7))),  # a one-layer slab at the box bottom (z_first = -1); the top slab's upper ghost is layer 0
    "A2": ("A", ((0, 5), (5, 7))),          # mz - owned = 2: each rank's two ghost layers are the other rank's end layers
    "B1": ("B", ((0, 3), (3, 6))),
    "B2": ("B", ((0, 2), (2, 4), (4, 6))),
    "C1": ("C", ((0, 4), (4, 8))),
}
LIST_QUIET_BUILDS = 4  # nl_api.hip: builds after which a handle leaves the launches for cells beyond the LDS buffer out
ROWS_CAP = {1: 1279, 2: 1663, 3: 2495}  # nl_rows.hpp: LDS stream of RowsCfg<fine_rows - 1>
gpu = pytest.mark.gpu


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def mesh(box):
    return tuple(int(b / RC) for b in box)


# ------------------------------------------------------------------------------------------------------ inputs


@functools.lru_cache(maxsize=None)
def make_input(box_name, per_cell, dtype_name, kind="uniform", extra=0):
    """Positions [n, 4] (read-only).  kind: "uniform"; "outside" (a tenth of the particles up to 0.9 box lengths outside on
    every side); "crowd" (`extra` more particles within +-0.9 rc of a point on the plane between the two slabs of the
    box's two-slab decomposition); "block" (`extra` more particles in each of the 3 x 3 x 3 cells whose z layers are the two
    below that plane and the one above it); "row_owned" / "row_ghost" (`extra` more particles along the row of x-cells (y, z) =
    (2, 2) / (2, mz - 1): for the slab [0, mz / 2) an owned row / a row of its lower, wrapped ghost layer)."""
    box = BOXES[box_name]
    dt = np.dtype(dtype_name).type
    m = mesh(box)
    n = per_cell * m[0] * m[1] * m[2]
    seed = 1000 * "ABCDE".index(box_name) + per_cell + (500 if dt == np.float64 else 0)
    q, _ = inputs.uniform_box(n, dtype=dt, seed=seed, box=box)
    rng = np.random.default_rng(seed + 7)
    ms = [b / k for b, k in zip(box, m)]
    if kind == "outside":
        k = n // 10
        q[:k, :3] += (rng.choice([-1.0, 1.0], size=(k, 3)) * rng.uniform(0.0, 0.9, size=(k, 3)) * np.array(box)).astype(dt)
    elif kind == "crowd":
        centre = np.array([0.5 * box[0], 0.5 * box[1], (m[2] // 2) * ms[2]])
        s = np.zeros((extra, 4), dtype=dt)
        s[:, :3] = (centre + rng.uniform(-0.9 * RC, 0.9 * RC, size=(extra, 3))).astype(dt)
        q = np.concatenate([q, s])
    elif kind == "block":  # rows of x-cells stay within their buckets, streams do not stay within the LDS buffer
        s = np.zeros((27 * extra, 4), dtype=dt)
        lo = (1, 1, m[2] // 2 - 2)
        for d in range(3):
            s[:, d] = ((lo[d] + rng.uniform(0.01, 2.99, len(s))) * ms[d]).astype(dt)
        q = np.concatenate([q, s])
    elif kind in ("row_owned", "row_ghost"):
        s = np.zeros((extra, 4), dtype=dt)
        s[:, 0] = rng.uniform(0.0, box[0] * (1 - 1e-6), extra)
        s[:, 1] = (2 + rng.uniform(0.05, 0.95, extra)) * ms[1]
        s[:, 2] = ((2 if kind == "row_owned" else m[2] - 1) + rng.uniform(0.05, 0.95, extra)) * ms[2]
        q = np.concatenate([q, s])
    else:
        assert kind == "uniform"
    q[:, 3] = 0
    q.setflags(write=False)
    return q


def slab_parts(q, box, rc, layers, mask=0):
    """Per (z_lo, z_hi) of `layers`: dict(z_lo, z_hi, own, glo, ghi, order = own ++ glo ++ ghi), input indices; glo is the
    layer (z_lo - 1) % mz, ghi the layer z_hi % mz (slab.z_layer: the library's own filing rule, which takes the floor
    where z is periodic and the reference's truncation where it is open)."""
    mz = int(box[2] / rc)
    iz = slab.z_layer(_torch().from_numpy(np.array(q)), box, rc, periodic_z=bool(mask & 4)).numpy()
    out = []
    for z_lo, z_hi in layers:
        own = np.nonzero((iz >= z_lo) & (iz < z_hi))[0]
        glo = np.nonzero(iz == (z_lo - 1) % mz)[0]
        ghi = np.nonzero(iz == z_hi % mz)[0]
        out.append(dict(z_lo=z_lo, z_hi=z_hi, own=own, glo=glo, ghi=ghi, order=np.concatenate([own, glo, ghi])))
    return out


# ------------------------------------------------------------------------------------------------------ expectations


def _canonical(kp, lst):
    """(counts, key_pointer, per-row ascending list) of a CSR."""
    kp = np.asarray(kp, dtype=np.int64)
    rows = np.repeat(np.arange(len(kp) - 1, dtype=np.int64), np.diff(kp))
    key = (rows << 32) | np.asarray(lst, dtype=np.int64)
    key.sort()
    return np.diff(kp), kp, (key & 0xFFFFFFFF).astype(np.int64)


def _symmetrised(kp, lst):
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    cols = np.asarray(lst, dtype=np.int64)
    a, b = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    cnt = np.bincount(a, minlength=n)
    return _canonical(np.concatenate([[0], np.cumsum(cnt)]), b[np.argsort(a, kind="stable")])


@functools.lru_cache(maxsize=None)
def global_list(key, mask, full):
    """(counts[n], key_pointer[n + 1], list) of the undivided box, per-row ascending, from the oracle alone.
    key: the arguments of make_input."""
    return list_of(make_input(*key), BOXES[key[0]], mask, full)


def list_of(q, box, mask, full):
    """global_list for any positions: (counts[n], key_pointer[n + 1], list), per-row ascending, from the oracle alone."""
    po = _po()
    if mask == 0:
        h = po.build(q, RC, box)
        return _symmetrised(h.key_pointer, h.sorted_list) if full else _canonical(h.key_pointer, h.sorted_list)
    if mask == 7:
        h = (po.build_pbc_full if full else po.build_pbc)(q, RC, box)
    else:
        h = padded_reference(q, RC, box, mask, full=full)
    return _canonical(h.key_pointer, h.sorted_list)


def take_rows(glob, rows):
    """(counts, list) of the rows `rows` of a global list, in that order."""
    cnt, kp, lst = glob
    c = cnt[rows]
    start = np.repeat(kp[rows] - (np.cumsum(c) - c), c)
    return c, lst[start + np.arange(int(c.sum()), dtype=np.int64)]


def mix_sum(row_ids, counts, lst):
    """The checksum of include/nl_hip.h (nl_list_checksum) in numpy: the wrapping sum of mix((id_i << 32) | j)."""
    v = (np.repeat(np.asarray(row_ids, dtype=np.uint64), counts) << np.uint64(32)) | np.asarray(lst, dtype=np.uint64)
    v = v * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    return int(v.sum(dtype=np.uint64))


def relabelled(glob_half, new_id, full):
    """The global list under ids new_id[i] (injective): half = every pair in the row of the smaller new id, full = the
    symmetrised list; rows indexed by particle, partners as new ids, ascending."""
    cnt, kp, lst = glob_half
    n = len(cnt)
    i = np.repeat(np.arange(n, dtype=np.int64), cnt)
    j = lst
    a, b = new_id[i], new_id[j]
    if full:
        rows, vals = np.concatenate([i, j]), np.concatenate([b, a])
    else:
        rows, vals = np.where(a < b, i, j), np.maximum(a, b)
    order = np.lexsort((vals, rows))
    c = np.bincount(rows, minlength=n)
    return c, np.concatenate([[0], np.cumsum(c)]), vals[order]


# ------------------------------------------------------------------------------------------------------ the library


def make_handle(box, n_max, dtype, mask=0, full=False, graph=False, capacity=None):
    """capacity: list entries for handles that build asynchronously (such a build cannot grow its list, and the default
    estimate takes the slab's particles over the volume of the whole box)."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(RC, *box, dtype=torch.float32 if np.dtype(dtype) == np.float32 else torch.float64, full_list=full)
    if mask:
        nl.set_periodic(axes=tuple(bool(mask >> d & 1) for d in range(3)))
    if graph:
        nl.set_graph(True)
    nl.Initialize(n_max)
    if capacity is not None:
        nl.set_capacity(int(capacity))
    return nl


def device_inputs(q, part, ids=None, form="gid4"):
    """(positions, gid argument) of MakeNeighListSlab for one slab.  ids: global id per input index (default: the index).
    form: "gid4" / "gid3" = explicit ids, position stride 4 / 3; "w" = ids in the w component (NL_GID_IN_W)."""
    torch = _torch()
    order = part["order"]
    gid = (order if ids is None else ids[order]).astype(np.int32)
    qa = np.array(q[order])
    if form == "gid3":
        qa = np.ascontiguousarray(qa[:, :3])
    if form == "w":
        qa[:, 3] = gid.view(np.float32) if qa.dtype == np.float32 else gid.astype(np.int64).view(np.float64)
        return torch.from_numpy(qa).cuda(), "w"
    return torch.from_numpy(qa).cuda(), torch.from_numpy(gid).cuda()


def read_slab(nl, wide=False):
    """The last slab build: per-row counts, key_pointer, per-row ascending partners (sorted on the device: plumbing),
    entries, checksum, build_info, build_stats."""
    torch = _torch()
    if nl.full_list:
        kp, lst, cnt = nl.full_csr(64 if wide else 32)
    else:
        kp, lst, cnt = (nl.key_pointer64() if wide else nl.key_pointer()), nl.sorted_list(), nl.half_number_of_partners()
    kp64 = kp.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(kp.shape[0] - 1, dtype=torch.int64, device=kp.device), kp64[1:] - kp64[:-1],
                                   output_size=int(lst.shape[0]))
    key, _ = torch.sort((rows << 32) | lst.to(torch.int64))
    cs, ne = nl.list_checksum()
    return dict(counts=cnt.cpu().numpy().astype(np.int64), key_pointer=kp.cpu().numpy().astype(np.int64),
                partners=(key & 0xFFFFFFFF).cpu().numpy(), entries=nl.list_entries(), half_pairs=nl.half_number_of_pairs(),
                checksum=cs, checksum_entries=ne, info=nl.build_info(), stats=nl.build_stats(), full=nl.full_list)


def build_slab(nl, q, part, ids=None, form="gid4", sync=True, split=False, wide=False, keep=None):
    """Runs MakeNeighListSlab (split: Begin + Finish) on one slab and reads it back (read_slab).  keep: a dict that holds
    the device tensors of (z_lo, z_hi) between calls, so that a captured graph is replayed with the same arguments."""
    k = (part["z_lo"], part["z_hi"], form)
    if keep is not None and k in keep:
        qa, gid = keep[k]
    else:
        qa, gid = device_inputs(q, part, ids, form)
        if keep is not None:
            keep[k] = (qa, gid)
    if split:
        nl.MakeNeighListSlabBegin(qa, gid, len(part["own"]), len(part["glo"]), part["z_lo"], part["z_hi"])
        nl.MakeNeighListSlabFinish(sync=sync)
    else:
        nl.MakeNeighListSlab(qa, gid, len(part["own"]), part["z_lo"], part["z_hi"], sync=sync)
    if not sync:
        nl.synchronize()
    return read_slab(nl, wide)


def check_rows(got, part, glob, what, ids=None):
    """Row r of the slab == row own[r] of the global list: counts, key_pointer, ascending partners, entry count, and the
    checksum of nl_hip.h over the rows' global ids.  Returns the checksum."""
    own = part["own"]
    want_c, want_l = take_rows(glob, own)
    bad = np.flatnonzero(got["counts"] != want_c)
    assert not len(bad), (f"{what}: slab [{part['z_lo']}, {part['z_hi']}) row {bad[0]} (particle {own[bad[0]]}) has "
                          f"{got['counts'][bad[0]]} partners, the oracle {want_c[bad[0]]}; {len(bad)} rows differ; {got['info']}")
    assert np.array_equal(got["key_pointer"], np.concatenate([[0], np.cumsum(want_c)])), what
    if not np.array_equal(got["partners"], want_l):
        k = int(np.flatnonzero(got["partners"] != want_l)[0])
        r = int(np.searchsorted(got["key_pointer"], k, side="right") - 1)
        raise AssertionError(f"{what}: slab [{part['z_lo']}, {part['z_hi']}) row {r} (particle {own[r]}): got "
                             f"{got['partners'][got['key_pointer'][r]:got['key_pointer'][r + 1]]}, the oracle "
                             f"{want_l[got['key_pointer'][r]:got['key_pointer'][r + 1]]}; {got['info']}")
    total = int(want_c.sum())
    assert got["entries"] == total and got["checksum_entries"] == total, what
    assert got["half_pairs"] == (total // 2 if got["full"] else total), what
    want_cs = mix_sum(own if ids is None else ids[own], want_c, want_l)
    assert got["checksum"] == want_cs, what
    return want_cs


def run_decomposition(nl, q, parts, glob, what, expect=None, **kw):
    """Every slab of a decomposition on one handle, each checked row by row; the checksums add up to the global list's.
    expect: build_info / build_stats values every slab must report (callables take the reported value)."""
    total = 0
    for part in parts:
        got = build_slab(nl, q, part, **kw)
        for name, want in (expect or {}).items():
            have = got["info"][name] if name in got["info"] else got["stats"][name]
            assert want(have) if callable(want) else have == want, (what, part["z_lo"], name, have, got["info"], got["stats"])
        assert got["info"]["id_classes"] == 0, (what, got["info"])
        total = (total + check_rows(got, part, glob, what, ids=kw.get("ids"))) & (2**64 - 1)
    cnt, _, lst = glob
    ids = kw.get("ids")
    assert total == mix_sum(np.arange(len(cnt)) if ids is None else ids, cnt, lst), what
    return total


def expected_plan(per_cell, dtype, mask):
    """What plan_build takes by default at the densities of this file (module docstring)."""
    f32_open = np.dtype(dtype) == np.float32 and mask == 0
    if per_cell == 8:
        return dict(masks=True, mask_rows=1, fine_rows=0, small_cells=1 if f32_open else 0)
    if per_cell == 30:
        return dict(masks=True, mask_rows=1, fine_rows=0, small_cells=0)
    if per_cell == 50:
        return dict(masks=True, mask_rows=2, fine_rows=2 if f32_open else 0, small_cells=0)
    assert per_cell == 90
    return dict(masks=True, mask_rows=3, fine_rows=0, small_cells=0)


def stencil_streams(q, part, box):
    """Stream length (particles of the 27 cells around it, periodic wrap) of every owned cell of a slab that holds some
    particle, from the oracle's cell ids of q[order]."""
    cell, m = _po().cells(np.ascontiguousarray(q[part["order"]]), RC, box)
    assert np.all(cell >= 0)
    cnt = np.bincount(cell, minlength=int(m[0] * m[1] * m[2])).reshape(m[2], m[1], m[0])
    tot = np.zeros_like(cnt)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                tot += np.roll(cnt, (dz, dy, dx), axis=(0, 1, 2))
    owned = tot[part["z_lo"]:part["z_hi"]]
    return owned[cnt[part["z_lo"]:part["z_hi"]] > 0]


# ------------------------------------------------------------------------------------------------------ CPU

CPU_INPUTS = ([(b, d, t, "uniform", 0) for b in "AB" for d in (8, 30, 50, 90) for t in ("float32", "float64")] +
              [("A", 30, "float32", "outside", 0), ("B", 30, "float64", "outside", 0),
               ("C", 8, "float32", "crowd", 1300), ("C", 25, "float64", "crowd", 1300), ("B", 50, "float32", "crowd", 1700),
               ("C", 8, "float32", "block", 60), ("C", 8, "float32", "row_owned", 600), ("C", 8, "float32", "row_ghost", 600)])


def test_decomposition_recipe_and_expectations_on_the_cpu():
    """The per-slab build emulated with the oracle on q[order] (mode "oracle" of tests/slab_worker.py) and the ownership
    rule, for every input of this file: the emulated rows are the rows cut out of the global list, every pair appears
    exactly once over the slabs, and the numpy checksum of the rows adds up to the oracle's hash of the global list."""
    po = _po()
    for key in CPU_INPUTS:
        q, box = make_input(*key), BOXES[key[0]]
        glob = global_list(key, 0, False)
        ref = po.build(q, RC, box)
        assert mix_sum(np.arange(len(q)), glob[0], glob[2]) == ref.hash(), key
        for name, (b, layers) in DECOMPS.items():
            if b != key[0]:
                continue
            parts = slab_parts(q, box, RC, layers)
            assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(len(q))), (key, name)
            seen, total = [], 0
            for p in parts:
                order, n_rows = p["order"], len(p["own"])
                h = po.build(np.ascontiguousarray(q[order]), RC, box)
                a = np.repeat(np.arange(len(order), dtype=np.int64), np.diff(h.key_pointer))
                b_ = h.sorted_list.astype(np.int64)
                ga, gb = order[a], order[b_]
                keep = np.where(ga < gb, a, b_) < n_rows  # the particle with the smaller global id is mine
                lo, hi = np.minimum(ga, gb)[keep], np.maximum(ga, gb)[keep]
                srt = np.lexsort((hi, lo))
                lo, hi = lo[srt], hi[srt]
                # rows in the order of own: own is ascending, so are the emulated rows
                want_c, want_l = take_rows(glob, p["own"])
                assert np.array_equal(np.bincount(np.searchsorted(p["own"], lo), minlength=n_rows), want_c), (key, name, p["z_lo"])
                assert np.array_equal(hi, want_l), (key, name, p["z_lo"])
                seen.append((lo << 32) | hi)
                total = (total + mix_sum(p["own"], want_c, want_l)) & (2**64 - 1)
            seen = np.concatenate(seen)
            assert len(np.unique(seen)) == len(seen) == ref.npairs, (key, name)
            assert total == ref.hash(), (key, name)


def test_relabelled_expectation_is_the_same_pair_set():
    """relabelled(): under new ids every pair of the oracle sits once, in the row of the smaller new id."""
    key = ("A", 30, "float32", "uniform", 0)
    glob = global_list(key, 0, False)
    new_id = scattered_ids(len(glob[0]), 3)
    assert new_id.min() == 0 and new_id.max() == 2**31 - 1 and len(np.unique(new_id)) == len(new_id)
    c, kp, vals = relabelled(glob, new_id, False)
    rows = np.repeat(np.arange(len(c)), c)
    assert np.all(new_id[rows] < vals)
    inv = {int(v): k for k, v in enumerate(new_id)}
    got = {(min(r, inv[int(v)]), max(r, inv[int(v)])) for r, v in zip(rows.tolist(), vals.tolist())}
    i = np.repeat(np.arange(len(c)), glob[0])
    assert got == set(zip(i.tolist(), glob[2].tolist())) and len(got) == len(vals)
    cf, _, vf = relabelled(glob, new_id, True)
    assert int(cf.sum()) == 2 * len(vals) and np.array_equal(cf, _symmetrised(glob[1], glob[2])[0])


def scattered_ids(n, seed):
    """A random injective map of n particles into [0, 2^31 - 1] that contains both ends."""
    rng = np.random.default_rng(seed)
    ids = np.unique(np.concatenate([[0, 2**31 - 1], rng.integers(1, 2**31 - 1, size=2 * n)]))
    inner = rng.choice(ids[1:-1], size=n - 2, replace=False)
    return rng.permutation(np.concatenate([[0, 2**31 - 1], inner])).astype(np.int64)


# ------------------------------------------------------------------------------------------------------ GPU


def _n_max(parts):
    return max(len(p["order"]) for p in parts)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("per_cell", [8, 30, 50, 90])
@pytest.mark.parametrize("decomp", ["A1", "A2", "B1", "B2"])
def test_default_plan_at_four_densities(decomp, per_cell, dtype):
    """Case 1: the plan's own choice at 8, 30, 50 and 90 particles per cell; masks 0 and 7, from 50 per cell on also 3 and
    4 (the multi-batch mask pipeline under a mixed mask); half and full list; every slab row by row."""
    box_name, layers = DECOMPS[decomp]
    key = (box_name, per_cell, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES[box_name]
    parts = slab_parts(q, box, RC, layers)
    for mask in (0, 7) + ((3, 4) if per_cell >= 50 else ()):
        nl = make_handle(box, _n_max(parts), dtype, mask)
        expect = dict(expected_plan(per_cell, dtype, mask), variant=3, offset_bits=32, cap_row=lambda v: v > 0)
        for full in (False, True):
            nl.set_full_list(full)
            run_decomposition(nl, q, parts, global_list(key, mask, full), (decomp, per_cell, dtype, mask, full), expect)


FORCED = [  # (environment, per cell, dtypes, masks, what build_info / build_stats must say)
    ({"NL_ROWS": "1"}, 30, ("float32",), (0,), dict(fine_rows=1)),
    ({"NL_ROWS": "2"}, 30, ("float32",), (0,), dict(fine_rows=2)),
    ({"NL_ROWS": "3"}, 30, ("float32",), (0,), dict(fine_rows=3)),
    ({"NL_ROWS": "4"}, 30, ("float32",), (0,), dict(fine_rows=1)),
    ({"NL_ROWS": "0"}, 30, ("float32",), (0,), dict(fine_rows=0, masks=True, mask_rows=1)),
    ({"NL_ROWS": "1"}, 50, ("float32",), (0,), dict(fine_rows=1)),  # streams beyond RowsCfg<0>'s LDS: k_rows_overflow
    ({"NL_ROWS": "3"}, 50, ("float32",), (0,), dict(fine_rows=3)),
    ({"NL_ROWS": "4"}, 50, ("float32",), (0,), dict(fine_rows=2)),
    ({"NL_ROWS": "0"}, 50, ("float32",), (0,), dict(fine_rows=0, masks=True, mask_rows=2)),  # fp32 open box, dense masks
    ({"NL_SWEEP_VARIANT": "1"}, 30, ("float32", "float64"), (0, 7), dict(variant=1, masks=False, fine_rows=0)),
    ({"NL_SWEEP_VARIANT": "1"}, 50, ("float32",), (0,), dict(variant=1, masks=False, fine_rows=0)),
    ({"NL_BINNING": "1"}, 30, ("float32", "float64"), (0, 7), dict(cap_row=0, fine_rows=0, masks=True)),
    ({"NL_BINNING": "1"}, 50, ("float32",), (0,), dict(cap_row=0, fine_rows=0, mask_rows=2)),  # no fine rows without the row binning
    ({"NL_BIN_BUCKETS": "0"}, 30, ("float32", "float64"), (0, 7), dict(cap_row=0, masks=True)),
    ({"NL_BIN_BUCKETS": "0"}, 50, ("float32",), (0,), dict(cap_row=0, fine_rows=2)),
    ({"NL_OFFSET_WIDTH": "64"}, 30, ("float32", "float64"), (0, 7), dict(offset_bits=64, masks=True)),
    ({"NL_OFFSET_WIDTH": "64"}, 50, ("float32", "float64"), (0,), dict(offset_bits=64, mask_rows=2)),
]


@gpu
@pytest.mark.parametrize("decomp", ["A1", "B1"])
@pytest.mark.parametrize("env,per_cell,dtypes,masks,expect", FORCED, ids=["-".join(f"{k}={v}" for k, v in f[0].items()) + f"-{f[1]}" for f in FORCED])
def test_forced_paths(env, per_cell, dtypes, masks, expect, decomp, monkeypatch):
    """Case 2: NL_ROWS, NL_SWEEP_VARIANT, NL_BINNING, NL_BIN_BUCKETS and NL_OFFSET_WIDTH, set before the handle exists;
    64-bit offsets are read through the csr64 getters and through the 32-bit ones."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    box_name, layers = DECOMPS[decomp]
    for dtype in dtypes:
        key = (box_name, per_cell, dtype, "uniform", 0)
        q, box = make_input(*key), BOXES[box_name]
        parts = slab_parts(q, box, RC, layers)
        for mask in masks:
            nl = make_handle(box, _n_max(parts), dtype, mask)
            for full in (False, True):
                nl.set_full_list(full)
                glob = global_list(key, mask, full)
                for wide in ((True, False) if "NL_OFFSET_WIDTH" in env else (False,)):
                    run_decomposition(nl, q, parts, glob, (env, decomp, per_cell, dtype, mask, full, wide), expect, wide=wide)


@gpu
@pytest.mark.parametrize("decomp,rows,mask,dtype", [(d, r, m, t) for d in ("A1", "B2") for r, m in ((None, 0), ("4", 0), (None, 7))
                                                    for t in ("float32", "float64") if not (r and t == "float64")])  # (fine rows: fp32 only)
def test_particles_outside_the_box(decomp, rows, mask, dtype, monkeypatch):
    """Case 3: a tenth of the particles up to 0.9 box lengths outside on every side; one with z < 0 is filed into a wrapped
    layer and owned by the rank of that layer."""
    if rows is not None:
        monkeypatch.setenv("NL_ROWS", rows)
    box_name, layers = DECOMPS[decomp]
    key = (box_name, 30, dtype, "outside", 0)
    q, box = make_input(*key), BOXES[box_name]
    assert (q[:, 2] < 0).any() and (q[:, 2] >= box[2]).any() and (q[:, 0] < 0).any() and (q[:, 1] >= box[1]).any()
    parts = slab_parts(q, box, RC, layers, mask)
    if mask & 4:  # some particle below the box lies in another layer than the open box's truncation files it into
        assert any(not np.array_equal(a["own"], b["own"]) for a, b in zip(parts, slab_parts(q, box, RC, layers)))
    nl = make_handle(box, _n_max(parts), dtype, mask)
    expect = dict(fine_rows=1) if rows else dict(fine_rows=0, masks=True, mask_rows=1)
    for full in (False, True):
        nl.set_full_list(full)
        run_decomposition(nl, q, parts, global_list(key, mask, full), (decomp, rows, mask, dtype, full), expect)


@gpu
@pytest.mark.parametrize("key,rows,expect", [
    (("C", 8, "float32", "crowd", 1300), None, dict(small_cells=1, masks=True, mask_rows=1, fine_rows=0)),
    (("C", 8, "float64", "crowd", 1300), None, dict(small_cells=0, masks=True, mask_rows=1)),
    (("C", 25, "float32", "crowd", 1300), None, dict(small_cells=0, masks=True, mask_rows=1, fine_rows=0)),
    (("C", 25, "float64", "crowd", 1300), None, dict(small_cells=0, masks=True, mask_rows=1)),
    (("B", 50, "float32", "crowd", 1700), "4", dict(fine_rows=lambda v: v > 0)),
])
def test_a_crowd_across_a_cut(key, rows, expect, monkeypatch):
    """Case 4: a crowd within +-0.9 rc of a point on the plane between two slabs: its cells are owned cells of one rank
    and ghost cells of the other.  In each slab some owned cell's stream exceeds the LDS batch (the hand-over to the
    batched search; with NL_ROWS=4 the fine-row buffer: k_rows_overflow) and some lies between half a batch and one."""
    if rows is not None:
        monkeypatch.setenv("NL_ROWS", rows)
    box = BOXES[key[0]]
    q = make_input(*key)
    parts = slab_parts(q, box, RC, DECOMPS["C1" if key[0] == "C" else "B1"][1])
    nl = make_handle(box, _n_max(parts), key[2])
    for full in (False, True):
        nl.set_full_list(full)
        glob = global_list(key, 0, full)
        for part in parts:
            got = build_slab(nl, q, part)
            for name, want in expect.items():
                assert want(got["info"][name]) if callable(want) else got["info"][name] == want, (key, name, got["info"])
            cap = ROWS_CAP[got["info"]["fine_rows"]] if rows else got["info"]["lds_batch"]
            streams = stencil_streams(q, part, box)
            assert (streams > cap).any(), (key, part["z_lo"], int(streams.max()), cap)
            if not rows:
                assert ((streams > cap // 2) & (streams <= cap)).any(), (key, part["z_lo"])
                assert got["stats"]["list_launched"]
            check_rows(got, part, glob, (key, rows, full))


@gpu
@pytest.mark.parametrize("sync", [True, False])
def test_quiet_slab_builds_then_a_crowd(sync):
    """Case 5a (tests/test_build_tail.py on a slab handle): after LIST_QUIET_BUILDS + 2 sparse builds the launches for cells
    beyond the LDS buffer are left out; the crowd slab (a block of 3 x 3 x 3 crowded cells across the cut, whose rows of
    x-cells stay within their buckets: a sphere-like crowd overflows those first and takes the other rerun) is run again
    with them, once, and is exact; the next build is exact without a further run."""
    box, layers = BOXES["C"], DECOMPS["C1"][1]
    sparse, crowd = ("C", 8, "float32", "uniform", 0), ("C", 8, "float32", "block", 60)
    q0, q1 = make_input(*sparse), make_input(*crowd)
    p0, p1 = slab_parts(q0, box, RC, layers)[0], slab_parts(q1, box, RC, layers)[0]
    nl = make_handle(box, len(p1["order"]), "float32", capacity=global_list(crowd, 0, False)[1][-1])
    for _ in range(LIST_QUIET_BUILDS + 2):
        got = build_slab(nl, q0, p0, sync=sync)
    check_rows(got, p0, global_list(sparse, 0, False), "sparse")
    assert not got["stats"]["list_launched"] and got["stats"]["list_reruns"] == 0 and got["info"]["small_cells"] == 1
    for _ in range(2):
        got = build_slab(nl, q1, p1, sync=sync)
        check_rows(got, p1, global_list(crowd, 0, False), "crowd")
        assert got["stats"]["list_reruns"] == 1 and got["stats"]["list_launched"], got["stats"]
        assert got["stats"]["row_overflow_reruns"] == 0, got["stats"]
    assert (stencil_streams(q1, p1, box) > got["info"]["lds_batch"]).any()


@gpu
@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("kind", ["row_owned", "row_ghost"])
def test_a_slab_row_past_its_bucket(kind, sync):
    """Case 5b: one row of x-cells crowded, in an owned layer and in the (wrapped) lower ghost layer: the build is run again
    with the two-pass binning, once, and is exact; the next build has larger buckets and needs no second run."""
    box, layers = BOXES["C"], DECOMPS["C1"][1]
    sparse, key = ("C", 8, "float32", "uniform", 0), ("C", 8, "float32", kind, 600)
    q0, q = make_input(*sparse), make_input(*key)
    p0, part = slab_parts(q0, box, RC, layers)[0], slab_parts(q, box, RC, layers)[0]
    assert np.isin(np.arange(len(q) - 600, len(q)), part["glo"] if kind == "row_ghost" else part["own"]).all()
    nl = make_handle(box, len(part["order"]), "float32", capacity=global_list(key, 0, False)[1][-1])
    first = build_slab(nl, q0, p0, sync=sync)
    check_rows(first, p0, global_list(sparse, 0, False), "sparse")
    assert first["stats"]["row_overflow_reruns"] == 0 and first["stats"]["cap_row"] > 0, first["stats"]
    got = build_slab(nl, q, part, sync=sync)
    check_rows(got, part, global_list(key, 0, False), kind)
    assert got["stats"]["row_overflow_reruns"] == 1, got["stats"]
    got = build_slab(nl, q, part, sync=sync)
    check_rows(got, part, global_list(key, 0, False), kind)
    assert got["stats"]["row_overflow_reruns"] == 1 and got["stats"]["cap_row"] >= 2 * first["stats"]["cap_row"] - 2, got["stats"]


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_id_forms_give_the_same_rows(dtype):
    """Case 6: explicit ids with position stride 4 and 3, and ids in the w component (int32 / int64 bit patterns)."""
    key = ("A", 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    nl = make_handle(box, _n_max(parts), dtype)
    for full in (False, True):
        nl.set_full_list(full)
        for form in ("gid4", "gid3", "w"):
            run_decomposition(nl, q, parts, global_list(key, 0, full), (dtype, full, form), form=form)


@gpu
@pytest.mark.parametrize("dtype,rows,per_cell", [("float32", None, 30), ("float64", None, 30), ("float32", "4", 50)])  # (fine rows: fp32 only)
def test_ids_that_are_not_a_permutation(dtype, rows, per_cell, monkeypatch):
    """Case 6: global ids scattered over [0, 2^31 - 1], both ends included: a pair sits in the row of the smaller new id."""
    if rows is not None:
        monkeypatch.setenv("NL_ROWS", rows)
    key = ("B", per_cell, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["B"]
    new_id = scattered_ids(len(q), 11)
    parts = slab_parts(q, box, RC, DECOMPS["B2"][1])
    nl = make_handle(box, _n_max(parts), dtype)
    for full in (False, True):
        nl.set_full_list(full)
        glob = relabelled(global_list(key, 0, False), new_id, full)
        for form in ("gid4", "w"):
            run_decomposition(nl, q, parts, glob, (dtype, rows, full, form), dict(fine_rows=(lambda v: v > 0) if rows else 0),
                              ids=new_id, form=form)


@gpu
@pytest.mark.parametrize("graph", [False, True])
def test_one_handle_many_slabs_and_graph_replay(graph):
    """Case 7: one handle builds the slabs of A1 in turn and again in reverse order (mzl, z_lo, n_rows and n all differ),
    asynchronously; with nl_set_graph the second round replays the captured graphs."""
    for dtype, full in (("float32", False), ("float32", True), ("float64", False)):
        key = ("A", 30, dtype, "uniform", 0)
        q, box = make_input(*key), BOXES["A"]
        parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
        nl = make_handle(box, _n_max(parts), dtype, full=full, graph=graph, capacity=global_list(key, 0, full)[1][-1])
        keep = {}
        for rnd in (parts, parts[::-1], parts):
            run_decomposition(nl, q, rnd, global_list(key, 0, full), (graph, dtype, full), sync=False, keep=keep)


@gpu
@pytest.mark.parametrize("env,per_cell,expect", [({"NL_ROWS": "4"}, 50, dict(fine_rows=2)), ({"NL_BINNING": "1"}, 30, dict(cap_row=0, fine_rows=0))])
def test_split_build_on_the_other_paths(env, per_cell, expect, monkeypatch):
    """Case 7: nl_make_list_slab_begin + _finish on the fine rows and on the atomic binning: the oracle's rows, as the
    single call gives them."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = ("B", per_cell, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["B"]
    parts = slab_parts(q, box, RC, DECOMPS["B2"][1])
    nl = make_handle(box, _n_max(parts), "float32")
    for full in (False, True):
        nl.set_full_list(full)
        for split in (True, False):
            run_decomposition(nl, q, parts, global_list(key, 0, full), (env, full, split), expect, split=split)


@gpu
@pytest.mark.parametrize("rows,per_cell,dtype", [(None, 30, "float32"), (None, 30, "float64"), ("4", 50, "float32")])
def test_misdescribed_slabs_are_refused(rows, per_cell, dtype, monkeypatch):
    """Case 8: an owned particle in a ghost layer, a ghost in an owned layer, a particle in a layer the slab does not hold:
    NL_ERR_DOMAIN each time, and the same handle then builds the correct slab exactly.  (Paths whose search kernels all
    read the status word before they walk the cell table: cell_setup_at for the 27-cell kernels, rows_windows for the
    fine rows.)"""
    from md_neighbor_list_amd._lib import NL_ERR_DOMAIN, NLError

    if rows is not None:
        monkeypatch.setenv("NL_ROWS", rows)
    key = ("B", per_cell, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["B"]
    ms_z = box[2] / mesh(box)[2]
    part = slab_parts(q, box, RC, DECOMPS["B2"][1])[1]  # layers [2, 4): ghosts 1 and 4, not held 0 and 5
    n_own, n_lo = len(part["own"]), len(part["glo"])
    nl = make_handle(box, len(part["order"]), dtype)
    glob = global_list(key, 0, False)
    expect = dict(fine_rows=2) if rows else dict(fine_rows=0, masks=True)
    for slot, z in ((5, 1.5 * ms_z), (5, 4.5 * ms_z), (n_own + 3, 2.5 * ms_z), (n_own + n_lo + 3, 3.5 * ms_z),
                    (7, 0.5 * ms_z), (n_own + 1, 5.5 * ms_z)):
        bad = np.array(q)
        bad[part["order"][slot], 2] = z
        with pytest.raises(NLError) as e:
            build_slab(nl, bad, part)
        assert e.value.code == NL_ERR_DOMAIN, (slot, z)
        run_decomposition_one(nl, q, part, glob, (rows, dtype, slot), expect)


def run_decomposition_one(nl, q, part, glob, what, expect):
    got = build_slab(nl, q, part)
    for name, want in expect.items():
        assert got["info"][name] == want, (what, name, got["info"])
    check_rows(got, part, glob, what)


@gpu
def test_transposed_list_refuses_a_slab():
    """nl_get_full_transposed indexes rows by id: a slab's full list, whose ids are global, has no transposed form
    (NL_ERR_STATE, include/nl_hip.h); the full CSR is the way to read it."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    part = slab_parts(q, box, RC, DECOMPS["A1"][1])[1]
    nl = make_handle(box, len(part["order"]), "float32", full=True)
    got = build_slab(nl, q, part)
    check_rows(got, part, global_list(key, 0, True), "full")
    with pytest.raises(NLError) as e:
        nl.neigh_list()
    assert e.value.code == NL_ERR_STATE
    with pytest.raises(NLError):
        nl.key_pointer()  # (the half getters refuse a full build, slab or not)

"""Builds at the mesh sizes where plan_build and its kernels change behaviour, row by row against the oracle.

The thresholds (md_neighbor_list_amd/csrc/nl_kernels.hpp, nl_api.hip), each met from both sides:

  BIN_MAX_MX = 4096, BIN_MAX_ROWS = 12288   two_level_ok: a mesh with more cells in a row of x-cells, or more rows, takes the
                                            atomic binning (k_hash, k_scan_chained over the cells, k_reorder) and has no
                                            id_rows, fine rows or id classes; at the limit the LDS tables of k_bin_rows,
                                            k_bin_scatter, k_bin_bucket and k_bin_cells are full to their last word
  BIN_FINE_MAX_MX = 2048                    the last mx of the fine rows and of four id classes (two classes: 4096)
  BC_KEEP * 256 = 1536 particles a row      beyond it k_bin_cells reads a row twice (the needles: 32768 to 81920 a row)
  1024 rows                                 beyond it a thread of the row scan of k_bin_scatter / k_bin_bucket has several
  64 look-back slots of k_scan_chained      block 65 and above take more than one step: more than 266 240 items

Shapes (mesh mx x my x mz, rc = 3.3, box (m + 0.4) rc per axis, uniform positions at `density` particles per cell, plus
five hand-placed pairs 0.5 rc apart -- SENTINELS):

  N2048, N2049   2048 / 2049 x 3 x 3    needles: 9 rows of x-cells
  N4096, N4097   4096 / 4097 x 3 x 3
  P12288         3 x 96 x 128           plates: exactly 12288 rows
  P12319         3 x 97 x 127           12319 rows
  P220           3 x 112 x 220          24640 rows; its halves have 12544 with their ghost layers, its thirds at most 8512
  S111           22 x 111 x 111         12321 rows, 271 062 cells: 67 scan blocks for the cells
  C65            65 x 65 x 65           4225 rows, 274 625 cells: 68 scan blocks

Every comparison is exact and against the oracle alone (list_of of tests/test_slab_paths.py): per-row counts, key_pointer,
per-row ascending partners, entry counts and nl_list_checksum.  Every GPU case asserts through build_info() /
build_stats() that the path it is for was taken; plan() restates plan_build's conditions in numpy, and the CPU tests
check that restatement against the values the GPU cases assert.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.test_slab_paths import (BOXES, RC, check_rows, list_of, make_handle, make_input, mix_sum, read_slab, run_decomposition,
                                   slab_parts)

gpu = pytest.mark.gpu

# restated from csrc/ (test_constants_are_the_sources)
BIN_MAX_ROWS, BIN_MAX_MX, BIN_FINE_MAX_MX = 12288, 4096, 2048
SCAN_SMALL_MAX, SCAN_BLOCK, SCAN_LOOK = 4096, 4096, 64
LEAN_SMALL_CAP, LDS_BATCH = 640, 1280

SHAPES = {"N2048": (2048, 3, 3), "N2049": (2049, 3, 3), "N4096": (4096, 3, 3), "N4097": (4097, 3, 3),
          "P12288": (3, 96, 128), "P12319": (3, 97, 127), "P220": (3, 112, 220), "S111": (22, 111, 111), "C65": (65, 65, 65)}
DENSITY = {"N2048": 8, "N2049": 8, "N4096": 8, "N4097": 8, "P12288": 8, "P12319": 8, "P220": 4, "S111": 1, "C65": 1}  # the lowest used
SENTINELS = ("last_x", "last_row", "x_face", "y_face", "z_face")  # pair k = particles n0 + 2 k, n0 + 2 k + 1
FACE_BIT = {"x_face": 1, "y_face": 2, "z_face": 4}


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def box_of(name):
    return tuple((m + 0.4) * RC for m in SHAPES[name])


def sentinels(name):
    """[10, 3] float64: five pairs 0.5 rc apart.  last_x: across the boundary between the last two x-cells; last_row: across
    the boundary between the last two rows of x-cells (y cells my - 2 | my - 1 of the top layer); x_ / y_ / z_face: through
    that face of the box, 0.25 rc inside on either side -- a pair where the axis is periodic, box - 0.5 rc apart where not."""
    m, box = SHAPES[name], box_of(name)
    ms = [b / k for b, k in zip(box, m)]
    h = 0.25 * RC
    mid = [1.5 * s for s in ms]
    out = np.empty((10, 3))
    out[0] = ((m[0] - 1) * ms[0] - h, mid[1], mid[2])
    out[1] = ((m[0] - 1) * ms[0] + h, mid[1], mid[2])
    out[2] = (mid[0], (m[1] - 1) * ms[1] - h, (m[2] - 0.5) * ms[2])
    out[3] = (mid[0], (m[1] - 1) * ms[1] + h, (m[2] - 0.5) * ms[2])
    for k, d in enumerate(range(3)):
        lo, hi = list(mid), list(mid)
        lo[d], hi[d] = h, box[d] - h
        lo[(d + 1) % 3] += 0.4  # (away from the other sentinels)
        hi[(d + 1) % 3] += 0.4
        out[4 + 2 * k], out[5 + 2 * k] = lo, hi
    return out


@functools.lru_cache(maxsize=None)
def shape_input(name, per_cell, dtype_name):
    """Positions [n0 + 10, 4] (read-only): n0 = per_cell * cells uniform ones, then the sentinel pairs."""
    m, box = SHAPES[name], box_of(name)
    dt = np.dtype(dtype_name).type
    n0 = per_cell * m[0] * m[1] * m[2]
    seed = 7000 + 100 * list(SHAPES).index(name) + per_cell + (50 if dt == np.float64 else 0)
    q, _ = inputs.uniform_box(n0, dtype=dt, seed=seed, box=box)
    s = np.zeros((10, 4), dtype=dt)
    s[:, :3] = sentinels(name).astype(dt)
    q = np.concatenate([q, s])
    q[:, 3] = 0
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=6)  # (a list of 4.6 M pairs is some 80 MB)
def shape_list(name, per_cell, dtype_name, mask, full):
    """(counts, key_pointer, per-row ascending list) of shape_input(...), from the oracle alone."""
    return list_of(shape_input(name, per_cell, dtype_name), box_of(name), mask, full)


def whole(q, m):
    """The undivided box as one 'slab' of check_rows: every row owned, in input order."""
    return dict(z_lo=0, z_hi=m[2], own=np.arange(len(q)))


def listed(glob, i, j):
    cnt, kp, lst = glob
    return bool((lst[kp[i]:kp[i + 1]] == j).any() or (lst[kp[j]:kp[j + 1]] == i).any())


# ------------------------------------------------------------------------------------------------------ plan_build in numpy


def plan(m, n, dtype, mask, full=False, env=None, mzl=None, n_max=None, slab=False, split=False):
    """What plan_build (nl_api.hip) chooses for a first build of n uniform particles on mesh m (mzl: the layers of a slab
    with its two ghost layers; split: Begin / Finish), in the words of build_info(): binning, fine_rows, id_classes,
    small_cells.  Restated for sparse boxes only (mean stencil stream within 0.85 LDS batches: the one-batch masks)."""
    env = env or {}
    f32 = np.dtype(dtype) == np.float32
    mx, my = m[0], m[1]
    mzl = m[2] if mzl is None else mzl
    n_max = n if n_max is None else n_max
    nrows = my * mzl
    stream = 27.0 * n / (mx * nrows)
    assert stream <= 0.85 * LDS_BATCH, "plan(): sparse boxes only"
    row_wise = env.get("NL_BINNING") != "1"
    two_level = row_wise and nrows <= BIN_MAX_ROWS and mx <= BIN_MAX_MX                                  # two_level_ok
    rows_layout = row_wise and nrows <= BIN_MAX_ROWS and mx <= BIN_FINE_MAX_MX and 4 * mx * nrows < 2147483000  # rows_layout_ok
    rows_margin = (m[2] + 0.4) / m[2] >= 1.0 + 8.0 * m[2] * 2.0**-24 + 2.0**-20                          # rows_margin_ok
    rows_env = int(env.get("NL_ROWS", -1))
    fine = rows_env if f32 and mask == 0 and 1 <= rows_env <= 3 and rows_layout and rows_margin else 0
    small = f32 and not fine and mask == 0 and stream + 5.0 * math.sqrt(stream) <= LEAN_SMALL_CAP
    cap = int(1.25 * n / nrows) + 256                                                                     # bucket_cap
    buckets = (not split and env.get("NL_BIN_BUCKETS") != "0" and two_level and
               nrows * cap + 16 <= 4 * (n_max + 16) + 512 * nrows)
    binning = "atomic" if not two_level else "bucket" if buckets else "two_pass"
    idc_env = {None: 2, "0": 0, "2": 2, "4": 4}[env.get("NL_IDCLASS")]
    idc = (f32 and not fine and not small and not full and mask == 0 and idc_env > 0 and not slab and binning != "atomic" and
           mx * idc_env <= 4 * BIN_FINE_MAX_MX and min(mx, my, mzl) >= 3 and n > 0)
    return dict(binning=binning, fine_rows=fine, id_classes=idc_env if idc else 0, small_cells=1 if small else 0)


def shape_plan(name, per_cell, dtype, mask, full=False, env=None):
    m = SHAPES[name]
    return plan(m, per_cell * m[0] * m[1] * m[2] + 10, dtype, mask, full, env)


# what the GPU cases below assert, spelled out (test_plan_restatement_gives_what_the_gpu_cases_assert)
ROW_TABLE_BINNING = {"N4096": "bucket", "N4097": "atomic", "P12288": "bucket", "P12319": "atomic"}
FINE_AND_CLASS_CASES = [  # (shape, per cell, environment, expected build_info values, list kinds)
    ("N2048", 8, {"NL_ROWS": "1"}, dict(fine_rows=1, binning="bucket", id_classes=0, small_cells=0), (False, True)),
    ("N2049", 8, {"NL_ROWS": "1"}, dict(fine_rows=0, binning="bucket", id_classes=0, small_cells=1), (False, True)),
    ("N2048", 20, {"NL_IDCLASS": "4"}, dict(id_classes=4, binning="bucket", fine_rows=0, small_cells=0), (False,)),
    ("N2049", 20, {"NL_IDCLASS": "4"}, dict(id_classes=0, binning="bucket", fine_rows=0, small_cells=0), (False,)),
    ("N4096", 20, {}, dict(id_classes=2, binning="bucket", fine_rows=0, small_cells=0), (False,)),
]
SCAN_CASES = [  # (shape, dtype, mask, environment, binning)
    ("S111", "float32", 0, {}, "atomic"), ("S111", "float32", 7, {}, "atomic"),
    ("S111", "float64", 0, {}, "atomic"), ("S111", "float64", 7, {}, "atomic"),
    ("S111", "float32", 0, {"NL_OFFSET_WIDTH": "64"}, "atomic"),
    ("C65", "float32", 0, {}, "bucket"), ("C65", "float32", 0, {"NL_BINNING": "1"}, "atomic"),
]
SLAB_CASES = {  # name: (shape, slabs, binning of one call, binning of Begin / Finish)
    "P12319-halves": ("P12319", ((0, 64), (64, 127)), "bucket", "two_pass"),
    "P220-halves": ("P220", ((0, 110), (110, 220)), "atomic", "atomic"),
    "P220-thirds": ("P220", ((0, 74), (74, 148), (148, 220)), "bucket", "two_pass"),
}
WALK = ("P12319", "P12288", "N4097", "S111")  # test_one_handle_across_the_limits
WALK_BINNING = {"B": "bucket", "P12319": "atomic", "P12288": "bucket", "N4097": "atomic", "S111": "atomic"}


# ------------------------------------------------------------------------------------------------------ CPU


def test_constants_are_the_sources():
    """The limits this file restates are those of csrc/: a changed limit fails here and names the shapes to move."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "md_neighbor_list_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("nl_kernels.hpp", "nl_lean.hpp", "nl_api.hip")}

    def const(f, name):
        found = re.findall(r"constexpr int " + name + r" = (\d+);", text[f])
        assert len(found) == 1, (f, name, found)
        return int(found[0])

    assert const("nl_kernels.hpp", "BIN_MAX_ROWS") == BIN_MAX_ROWS, "move P12288 / P12319 / S111 and the slabs of P220"
    assert const("nl_kernels.hpp", "BIN_MAX_MX") == BIN_MAX_MX, "move N4096 / N4097"
    assert const("nl_kernels.hpp", "BIN_FINE_MAX_MX") == BIN_FINE_MAX_MX, "move N2048 / N2049"
    assert const("nl_kernels.hpp", "SCAN_SMALL_MAX") == SCAN_SMALL_MAX
    assert const("nl_kernels.hpp", "SCAN_THREADS") * const("nl_kernels.hpp", "SCAN_ITEMS") == SCAN_BLOCK, "move S111 / C65"
    assert re.search(r"constexpr int SCAN_BLOCK = SCAN_THREADS \* SCAN_ITEMS;", text["nl_kernels.hpp"])
    caps = re.findall(r"struct SweepCfg<(?:float|double)> \{ static constexpr int CAP = (\d+); \}", text["nl_kernels.hpp"])
    assert caps == [str(LDS_BATCH)] * 2, caps
    assert re.search(r"constexpr int LEAN_SMALL_CAP = SweepCfg<float>::CAP / 2;", text["nl_lean.hpp"]) and LEAN_SMALL_CAP == LDS_BATCH // 2
    # the conditions plan() restates, as nl_api.hip writes them
    for cond in ("(int64_t)h->m[1] * mzl <= BIN_MAX_ROWS && h->m[0] <= BIN_MAX_MX", "h->m[0] <= BIN_FINE_MAX_MX",
                 "h->m[0] * h->idclass_env <= 4 * BIN_FINE_MAX_MX", "mean_stream + 5.0 * std::sqrt(mean_stream) <= (double)LEAN_SMALL_CAP"):
        assert cond in text["nl_api.hip"], cond


def test_shapes_are_the_named_meshes():
    """int(b / rc) gives the named mesh; rows, cells and scan blocks are what the module docstring claims."""
    for name, m in SHAPES.items():
        assert tuple(int(b / RC) for b in box_of(name)) == m, name
    rows = {k: m[1] * m[2] for k, m in SHAPES.items()}
    cells = {k: m[0] * m[1] * m[2] for k, m in SHAPES.items()}
    assert rows["P12288"] == BIN_MAX_ROWS and rows["P12319"] == 12319 and rows["S111"] == 12321 and rows["C65"] == 4225
    assert rows["P220"] == 24640 and all(rows[k] == 9 for k in ("N2048", "N2049", "N4096", "N4097"))
    assert cells["S111"] == 271062 and cells["C65"] == 274625 and cells["P220"] * 4 == 295680 and cells["N4096"] * 20 == 737280
    # the chained scan: a block numbered 65 or higher looks back more than SCAN_LOOK blocks
    for k, blocks in (("S111", 67), ("C65", 68)):
        assert -(-cells[k] // SCAN_BLOCK) == blocks and blocks - 1 > SCAN_LOOK and cells[k] > SCAN_SMALL_MAX, k
    for k in SHAPES:  # beyond 2048 cells a row the counts (one per particle) take the scan beyond one look-back step as well
        assert k in ("N2048", "N2049") or DENSITY[k] * cells[k] > (SCAN_LOOK + 1) * SCAN_BLOCK, k
    # the needles' rows take the read-twice branch of k_bin_cells; the plates and cubes give a scan thread several rows
    assert all(DENSITY[k] * SHAPES[k][0] * 1 > 1536 for k in ("N2048", "N2049", "N4096", "N4097"))
    assert all(rows[k] > 1024 for k in ("P12288", "C65")) and all(SHAPES[k][1] * z > 1024 for k, z in (("P12319", 66), ("P220", 74)))
    for name, (shape, layers, _, _) in SLAB_CASES.items():
        m = SHAPES[shape]
        assert layers[0][0] == 0 and layers[-1][1] == m[2] and all(a[1] == b[0] for a, b in zip(layers, layers[1:])), name
    assert [(hi - lo + 2) * 112 for lo, hi in SLAB_CASES["P220-halves"][1]] == [12544, 12544]
    assert max((hi - lo + 2) * 112 for lo, hi in SLAB_CASES["P220-thirds"][1]) == 8512
    assert [(hi - lo + 2) * 97 for lo, hi in SLAB_CASES["P12319-halves"][1]] == [6402, 6305]


def test_plan_restatement_gives_what_the_gpu_cases_assert():
    """two_level_ok, rows_layout_ok, the id-class condition and `small` in numpy, for every GPU case of this file."""
    for name, binning in ROW_TABLE_BINNING.items():
        for dtype in ("float32", "float64"):
            for mask in (0, 7):
                for full in (False, True):
                    want = dict(binning=binning, fine_rows=0, id_classes=0, small_cells=1 if dtype == "float32" and mask == 0 else 0)
                    assert shape_plan(name, 8, dtype, mask, full) == want, (name, dtype, mask, full)
    for name in ("N4096", "P12288"):
        for dtype in ("float32", "float64"):
            assert shape_plan(name, 8, dtype, 0, env={"NL_BIN_BUCKETS": "0"})["binning"] == "two_pass"
    for name, per_cell, env, want, kinds in FINE_AND_CLASS_CASES:
        for full in kinds:
            assert shape_plan(name, per_cell, "float32", 0, full, env) == want, (name, per_cell, env, full)
    # both sides of each mx limit: 2048 | 2049 for the fine rows and four classes, 4096 | 4097 for two classes and the rows
    assert shape_plan("N4097", 20, "float32", 0)["id_classes"] == 0 and shape_plan("N4096", 20, "float32", 0, env={"NL_IDCLASS": "4"})["id_classes"] == 0
    assert 27 * 20 + 5 * math.sqrt(27 * 20) > LEAN_SMALL_CAP >= 27 * 8 + 5 * math.sqrt(27 * 8)  # 20 per cell: no small cells, so id classes
    for name, dtype, mask, env, binning in SCAN_CASES:
        got = shape_plan(name, 1, dtype, mask, env=env)
        assert got["binning"] == binning and got["fine_rows"] == 0 and got["id_classes"] == 0, (name, dtype, mask, env)
        assert got["small_cells"] == (1 if dtype == "float32" and mask == 0 else 0)
    for name in ("N4097", "P12319", "S111"):
        for n in (0, 1, 2):
            assert plan(SHAPES[name], n, "float32", 0, n_max=16)["binning"] == "atomic"
    for name, (shape, layers, one_call, begin_finish) in SLAB_CASES.items():
        m, per_cell = SHAPES[shape], DENSITY[shape]
        assert shape_plan(shape, per_cell, "float32", 0)["binning"] == "atomic", name
        for lo, hi in layers:
            n = per_cell * m[0] * m[1] * (hi - lo + 2)
            for split, want in ((False, one_call), (True, begin_finish)):
                got = plan(m, n, "float32", 0, mzl=hi - lo + 2, slab=True, split=split)
                assert got["binning"] == want and got["id_classes"] == 0, (name, lo, hi, split)
    for name in WALK:
        assert plan(SHAPES[name], DENSITY[name] * int(np.prod(SHAPES[name])) + 10, "float32", 7, n_max=300000)["binning"] == WALK_BINNING[name]
    assert plan((5, 4, 6), 960, "float32", 7, n_max=300000)["binning"] == WALK_BINNING["B"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_sentinel_pairs_in_the_oracle_lists(name):
    """The hand-placed pairs lie where they are meant to and the oracle lists them: across the last cell boundary of x
    and across the last row boundary under every mask, through a face only where that face is periodic."""
    m, box = SHAPES[name], box_of(name)
    q = shape_input(name, DENSITY[name], "float32")
    n0 = len(q) - 10
    cell, mesh = _po().cells(q, RC, box)
    assert tuple(mesh) == m
    cx, row = cell % m[0], cell // m[0]
    assert (cx[n0], cx[n0 + 1]) == (m[0] - 2, m[0] - 1) and row[n0] == row[n0 + 1], name
    assert (row[n0 + 2], row[n0 + 3]) == (m[1] * m[2] - 2, m[1] * m[2] - 1) and cx[n0 + 2] == cx[n0 + 3], name
    assert (cx[n0 + 4], cx[n0 + 5]) == (0, m[0] - 1), name
    assert (row[n0 + 6] % m[1], row[n0 + 7] % m[1]) == (0, m[1] - 1), name
    assert (row[n0 + 8] // m[1], row[n0 + 9] // m[1]) == (0, m[2] - 1), name
    open_box, periodic = shape_list(name, DENSITY[name], "float32", 0, False), shape_list(name, DENSITY[name], "float32", 7, False)
    for k, what in enumerate(SENTINELS):
        i, j = n0 + 2 * k, n0 + 2 * k + 1
        assert listed(periodic, i, j), (name, what)
        assert listed(open_box, i, j) == (what not in FACE_BIT), (name, what)


def test_each_limit_is_populated_in_the_oracle_lists():
    """Pairs in x-cell 4096 of N4097, in x-cell 4095 of N4096, in rows >= 12288 of P12319; under mask 7 pairs through the
    x faces of the needles and through the y and z faces of the plates (uniform particles, not only the sentinels)."""
    def rows_with_pairs(name, mask):
        q = shape_input(name, 8, "float32")
        cell, _ = _po().cells(q, RC, box_of(name))
        return q, cell, shape_list(name, 8, "float32", mask, False)

    q, cell, (cnt, kp, lst) = rows_with_pairs("N4097", 0)
    assert cnt[cell % 4097 == 4096].sum() > 0
    q, cell, (cnt, kp, lst) = rows_with_pairs("N4096", 0)
    assert cnt[cell % 4096 == 4095].sum() > 0
    q, cell, (cnt, kp, lst) = rows_with_pairs("P12319", 0)
    assert cnt[cell // 3 >= BIN_MAX_ROWS].sum() > 0 and (cell // 3).max() == 12318
    for name, axes in (("N4096", (0,)), ("N4097", (0,)), ("P12288", (1, 2)), ("P12319", (1, 2))):
        q, cell, (cnt, kp, lst) = rows_with_pairs(name, 7)
        n0 = len(q) - 10
        i = np.repeat(np.arange(len(q)), cnt)
        both_uniform = (i < n0) & (lst < n0)
        d = np.abs(q[i, :3].astype(np.float64) - q[lst, :3].astype(np.float64))
        for axis in axes:
            assert ((d[:, axis] > 0.5 * box_of(name)[axis]) & both_uniform).any(), (name, axis)


@pytest.mark.parametrize("name", ["N4097", "P12319"])
def test_a_list_without_the_rows_beyond_the_limit_has_another_checksum(name):
    """Teeth: the oracle's list of the same positions without the particles of the last x-cell (N4097), of the rows >=
    12288 (P12319), has another checksum, by mix_sum and by HalfList.hash()."""
    po, box, m = _po(), box_of(name), SHAPES[name]
    q = shape_input(name, 8, "float32")
    cell, _ = po.cells(q, RC, box)
    beyond = (cell % m[0] == BIN_MAX_MX) if name == "N4097" else (cell // m[0] >= BIN_MAX_ROWS)
    assert 0 < beyond.sum() < len(q) // 100
    cut = np.ascontiguousarray(q[~beyond])
    cnt, kp, lst = shape_list(name, 8, "float32", 0, False)
    cnt2, kp2, lst2 = list_of(cut, box, 0, False)
    assert kp2[-1] < kp[-1], name
    assert mix_sum(np.arange(len(cnt)), cnt, lst) != mix_sum(np.arange(len(cnt2)), cnt2, lst2), name
    assert po.build_pbc(q, RC, box).hash() != po.build_pbc(cut, RC, box).hash(), name


# ------------------------------------------------------------------------------------------------------ GPU


def build_whole(nl, q, wide=False):
    torch = _torch()
    qd = torch.from_numpy(np.array(q)).cuda()
    nl.MakeNeighList(qd, len(q))
    return read_slab(nl, wide)


def check_whole(got, q, m, glob, what, expect):
    """build_info() / build_stats() say what `expect` does; then every row against the oracle (check_rows)."""
    for key, want in expect.items():
        have = got["info"][key] if key in got["info"] else got["stats"][key]
        assert want(have) if callable(want) else have == want, (what, key, have, got["info"], got["stats"])
    binning = got["info"]["binning"]
    assert (got["stats"]["cap_row"] > 0) == (binning == "bucket"), (what, got["info"], got["stats"])
    if binning == "atomic":
        assert got["info"]["fine_rows"] == 0 and got["info"]["id_classes"] == 0, (what, got["info"])
    return check_rows(got, whole(q, m), glob, what)


@gpu
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", list(ROW_TABLE_BINNING))
def test_row_table_limits_default_plan(name, dtype, mask):
    """Case 1: 4096 | 4097 cells in a row, 12288 | 12319 rows, at 8 per cell: the row tables full to the last word on one
    side (bucket binning), the atomic binning on the other; half and full list."""
    q, m = shape_input(name, 8, dtype), SHAPES[name]
    nl = make_handle(box_of(name), len(q), dtype, mask)
    assert tuple(nl.mesh_size) == m
    expect = dict(binning=ROW_TABLE_BINNING[name], fine_rows=0, id_classes=0, masks=True, mask_rows=1, offset_bits=32,
                  small_cells=1 if dtype == "float32" and mask == 0 else 0)
    for full in (False, True):
        nl.set_full_list(full)
        check_whole(build_whole(nl, q), q, m, shape_list(name, 8, dtype, mask, full), (name, dtype, mask, full), expect)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["N4096", "P12288"])
def test_row_table_limits_two_pass(name, dtype, monkeypatch):
    """Case 1, NL_BIN_BUCKETS=0: k_bin_rows / k_bin_scatter with full tables; in fp32 the cell table is the oracle's cell
    histogram prefix."""
    monkeypatch.setenv("NL_BIN_BUCKETS", "0")
    q, m = shape_input(name, 8, dtype), SHAPES[name]
    nl = make_handle(box_of(name), len(q), dtype, 0)
    got = build_whole(nl, q)
    check_whole(got, q, m, shape_list(name, 8, dtype, 0, False), (name, dtype), dict(binning="two_pass", cap_row=0, fine_rows=0, id_classes=0))
    if dtype == "float32":
        cell, _ = _po().cells(q, RC, box_of(name))
        want = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=m[0] * m[1] * m[2]))])
        cell_start = nl.sorted_state()[0].cpu().numpy()
        assert cell_start.shape == want.shape, (name, cell_start.shape)
        bad = np.flatnonzero(cell_start != want)
        assert not len(bad), f"{name}: cell_start[{bad[0]}] (cell x {bad[0] % m[0]}, row {bad[0] // m[0]}) = {cell_start[bad[0]]}, the oracle {want[bad[0]]}"


@gpu
@pytest.mark.parametrize("name,per_cell,env,expect,kinds", FINE_AND_CLASS_CASES,
                         ids=[f"{c[0]}-{c[1]}-" + ("-".join(f"{k}={v}" for k, v in c[2].items()) or "default") for c in FINE_AND_CLASS_CASES])
def test_fine_rows_and_id_classes_at_their_last_mesh(name, per_cell, env, expect, kinds, monkeypatch):
    """Case 2: fp32, open box.  2048 cells a row is the last mesh of the fine rows (cnt[4 * 2048] of k_bin_cells<FINE>) and
    of four id classes, 4096 the last of two; one cell more and the build goes without."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    q, m = shape_input(name, per_cell, "float32"), SHAPES[name]
    nl = make_handle(box_of(name), len(q), "float32", 0)
    for full in kinds:
        nl.set_full_list(full)
        check_whole(build_whole(nl, q), q, m, shape_list(name, per_cell, "float32", 0, full), (name, per_cell, env, full), dict(expect, masks=True))


@gpu
@pytest.mark.parametrize("name,dtype,mask,env,binning", SCAN_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-" + ("-".join(f"{k}={v}" for k, v in c[3].items()) or "default") for c in SCAN_CASES])
def test_long_scans(name, dtype, mask, env, binning, monkeypatch):
    """Case 3: more than 65 scan blocks of cells at 1 per cell: k_scan_chained beyond one look-back step over the cell
    histogram of the atomic binning (S111; C65 under NL_BINNING=1), over the counts of every build; 64-bit offsets through
    both getters."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wide = env.get("NL_OFFSET_WIDTH") == "64"
    q, m = shape_input(name, 1, dtype), SHAPES[name]
    nl = make_handle(box_of(name), len(q), dtype, mask)
    expect = dict(binning=binning, fine_rows=0, id_classes=0, offset_bits=64 if wide else 32, masks=True,
                  small_cells=1 if dtype == "float32" and mask == 0 else 0)
    got = build_whole(nl, q, wide)
    check_whole(got, q, m, shape_list(name, 1, dtype, mask, False), (name, dtype, mask, env), expect)
    if wide:
        check_whole(read_slab(nl, False), q, m, shape_list(name, 1, dtype, mask, False), (name, dtype, mask, env, "32-bit getter"), expect)


@gpu
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("name", ["N4097", "P12319", "S111"])
def test_empty_and_nearly_empty(name, mask):
    """Case 4: no particle, one, and the two of the sentinel pair through the x face, on the meshes beyond the row tables:
    cell tables of up to 271 062 entries, all but one or two empty."""
    m, box = SHAPES[name], box_of(name)
    q = shape_input(name, DENSITY[name], "float32")
    n0 = len(q) - 10
    nl = make_handle(box, 16, "float32", mask)
    for rows, pairs in ((np.arange(0), 0), (np.array([n0 // 2]), 0), (np.array([n0 + 4, n0 + 5]), 1 if mask else 0)):
        sub = np.ascontiguousarray(q[rows]).reshape(len(rows), 4)
        glob = list_of(sub, box, mask, False)
        assert glob[1][-1] == pairs, (name, mask, len(rows))
        check_whole(build_whole(nl, sub), sub, m, glob, (name, mask, len(rows)), dict(binning="atomic", fine_rows=0, id_classes=0))


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["one-call", "begin-finish"])
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", list(SLAB_CASES))
def test_slabs_across_the_row_limit(case, dtype, mask, split):
    """Case 5: the whole box is beyond the row tables, a slab of it is not (P12319 halves, P220 thirds) or is as well (P220
    halves): two_level_ok depends on the slab's layers.  Row by row; the slabs' checksums add up to the global list's."""
    name, layers, one_call, begin_finish = SLAB_CASES[case]
    per_cell, m, box = DENSITY[name], SHAPES[name], box_of(name)
    q = shape_input(name, per_cell, dtype)
    glob = shape_list(name, per_cell, dtype, mask, False)
    parts = slab_parts(q, box, RC, layers, mask)
    nl = make_handle(box, len(q), dtype, mask)
    if not split:  # the undivided box first, on the same handle
        check_whole(build_whole(nl, q), q, m, glob, (case, dtype, mask, "whole"), dict(binning="atomic"))
    expect = dict(binning=begin_finish if split else one_call, fine_rows=0)
    run_decomposition(nl, q, parts, glob, (case, dtype, mask, split), expect, split=split)


@gpu
def test_one_handle_across_the_limits():
    """Case 6: nl_set_box moves one handle from 5 x 4 x 6 cells to 12319 rows, 12288 rows, 4097 cells a row, 271 062 cells
    and back (reserve_mesh regrows the buffers and moves the status word): after each, the oracle's list and the binning of
    a fresh handle."""
    key = ("B", 8, "float32", "uniform", 0)
    nl = make_handle(BOXES["B"], 300000, "float32", 7)
    steps = [("B", make_input(*key), BOXES["B"], (5, 4, 6))]
    steps += [(name, shape_input(name, DENSITY[name], "float32"), box_of(name), SHAPES[name]) for name in WALK]
    steps.append(steps[0])
    for k, (name, q, box, m) in enumerate(steps):
        if k:
            nl.set_box(*box)
        assert tuple(nl.mesh_size) == m, (k, name, nl.mesh_size)
        glob = list_of(q, box, 7, False) if name == "B" else shape_list(name, DENSITY[name], "float32", 7, False)
        check_whole(build_whole(nl, q), q, m, glob, (k, name), dict(binning=WALK_BINNING[name], fine_rows=0, id_classes=0))


@gpu
def test_update_on_the_large_atomic_mesh():
    """Case 7: nl_update_list on S111 (atomic binning, 67 scan blocks of cells), skin 0.6: the first update builds, the same
    positions skip and leave every array byte for byte, one interior particle moved by 1.1 skin / 2 builds again."""
    from tests.test_update_paths import raw_state, same_state

    torch = _torch()
    name, skin = "S111", 0.6
    m, box = SHAPES[name], box_of(name)
    q0 = shape_input(name, 1, "float32")
    nl = make_handle(box, len(q0), "float32", 0)
    nl.set_skin(skin)
    expect = dict(binning="atomic", cap_row=0, list_launched=True, small_cells=1)
    qd = torch.from_numpy(np.array(q0)).cuda()
    nl.update(qd, sync=True)
    check_whole(read_slab(nl), q0, m, shape_list(name, 1, "float32", 0, False), "first update", expect)
    assert nl.update_stats() == (1, 1)
    before = raw_state(nl, False)
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 1)
    same_state(before, raw_state(nl, False), "the same positions again")
    check_whole(read_slab(nl), q0, m, shape_list(name, 1, "float32", 0, False), "skipped update", expect)
    inside = np.flatnonzero(np.all((q0[:, :3] > 2 * RC) & (q0[:, :3] < np.array(box) - 2 * RC), axis=1))[0]
    q1 = np.array(q0)
    q1[inside, 0] += np.float32(1.1 * skin / 2)
    assert (float(q1[inside, 0]) - float(q0[inside, 0])) ** 2 > (skin / 2) ** 2
    qd.copy_(torch.from_numpy(q1))
    nl.update(qd, sync=True)
    check_whole(read_slab(nl), q1, m, list_of(q1, box, 0, False), "moved particle", expect)
    assert nl.update_stats() == (3, 2)

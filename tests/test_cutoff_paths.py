"""The cut-off decision at the last bit on every search path.

A pair is in the list iff !(r2 > rc2), r2 = (dx*dx + dy*dy) + dz*dz rounded operation by operation in the position type
(include/nl_hip.h).  plan_build chooses among about ten search kernels, and several reach that decision by a shortcut that
is sound only by an error analysis: the fp32 screen of the fp64 search, the quarter-plane reach of the fine rows, the id
classes, the rounded face shifts and the three binning kernels that store a wrapped particle's image.  Uniform random input
has no pair within thousands of ulp of rc2, so here every path is built on the clouds of tests/cutoff_util.py -- pairs at
rc (1 + k ulp) in the corners of their cells, on the quarter-planes, across the faces, a box length outside and inside a
crowded cell -- and compared with the oracle of the same rule: number_of_partners, key_pointer, the canonical list and the
checksum, half and full list (with a mask the full references, where each row decides on its own).  Every device test first
asserts through build_info() / build_stats() that the path it is meant for was the one taken.

The unmarked tests check the input itself on the CPU: per cloud and class, at least 25 constructed pairs accepted and 25
rejected within 16 ulp of rc2 by the header's rule (and, for `zplane`, at least 10 accepted pairs exactly 3 and exactly 4
quarter-planes apart in each z direction), and that rule agrees with the oracle's list on every constructed pair.
"""
import functools
import os
import re
import zlib

import numpy as np
import pytest

from tests import cutoff_util as cu
from tests.cutoff_util import BOX, RC

gpu = pytest.mark.gpu
F32, F64 = "float32", "float64"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "md_neighbor_list_amd", "csrc")


def source_constant(file, pattern):
    """An integer constant of the kernels, read from their source: a test that depends on one follows it when it changes."""
    with open(os.path.join(CSRC, file)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, (file, pattern, found)
    return int(found[0])


# LDS stream of RowsCfg<0>: a cell beyond it goes to k_rows_overflow
ROWS0_CAP = source_constant("nl_rows.hpp", r"struct RowsCfg<0> \{ static constexpr int CAP = (\d+)")
# builds after which a handle leaves the launches for cells beyond the LDS batch out
LIST_QUIET_BUILDS = source_constant("nl_api.hip", r"constexpr int32_t LIST_QUIET_BUILDS = (\d+);")
FACES = ("face_x", "face_y", "face_z")


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def open_outside(mask):
    return tuple(name for name, a in cu.OUTSIDE.items() if not mask >> a & 1)


def margin_box(above):
    """BOX with an Lz that puts ms_z / rc about 2^-30 (relative) above / below the threshold of rows_margin_ok
    (nl_api.hip), computed with the same double expression."""
    mz = 5
    thr = 1.0 + 8.0 * mz * 2.0 ** -24 + 2.0 ** -20
    Lz = mz * RC * thr * (1.0 + (2.0 ** -30 if above else -(2.0 ** -30)))
    assert int(Lz / RC) == mz and ((Lz / mz) / RC >= thr) == above
    assert abs((Lz / mz) / RC / thr - 1.0) < 2.0 ** -29
    return (BOX[0], BOX[1], Lz)


# ------------------------------------------------------------------------------------------------------ the cases
# (dtype, mask, classes, particles per cell, box, signed) of every cloud the device tests build; the self-checks run over all
# of them.  signed (mixed masks): the cloud has negative open-axis coordinates -- outside_* by -L as well as +L, partners left
# below a low open face -- and its reference is cutoff_util.brute_force; the unsigned mixed-mask clouds keep to what the
# padded reference of tests/test_periodic_axes.py admits.  Both kinds are built.

CASES = {}


def GROUPS(mask):
    """The classes of the builds with a mask -- random, corners, every face, and a box length outside on the open axes -- a
    few to a cloud, so that the background keeps its share of the particles."""
    return [("rand", "corner"), FACES] + ([open_outside(mask)] if mask != 7 else [])


def case(name, dtype, mask, classes, per_cell, box=BOX, signed=False):
    CASES.setdefault(name, []).append((dtype, mask, tuple(classes), float(per_cell), tuple(box), bool(signed)))


# the 2-wave instance: one class a cloud and 16 particles per cell in all (10.7 of them background).  plan_build takes it
# while the mean stencil stream + 5 sigma stays within half the LDS batch, i.e. up to 19.6 per cell counting the 800
# constructed particles, so the background cannot be denser with 400 pairs a class
for _c in ("rand", "corner") + FACES + open_outside(0):
    case("lean", F32, 0, (_c,), 16)
for _dt in (F32, F64):
    for _m in (0, 5, 7):
        for _g in GROUPS(_m):
            case(f"masks-{_dt}-{_m}", _dt, _m, _g, 30)
    for _g in GROUPS(5)[1:]:
        case(f"masks-{_dt}-5", _dt, 5, _g, 30, signed=True)
    for _m in (0, 7):
        for _g in GROUPS(_m)[:2]:
            case(f"dense-{_dt}-{_m}", _dt, _m, _g, 50)
    case(f"list-{_dt}", _dt, 0, ("cluster",), 30)
    for _m in (0, 7):
        for _g in [("rand", "corner", "cut")] + GROUPS(_m)[1:]:
            case(f"slab-{_dt}-{_m}", _dt, _m, _g, 30)
case("idclass", F32, 0, ("rand", "corner", "zplane"), 30)
for _g in (("rand", "corner", "zplane"), open_outside(0)):
    case("rows-30", F32, 0, _g, 30)
    case("rows-50", F32, 0, _g, 50)
case("rows-overflow", F32, 0, ("cluster", "zplane"), 30)
case("margin-above", F32, 0, ("zplane",), 30, margin_box(True))
case("margin-below", F32, 0, ("zplane",), 30, margin_box(False))
ALL_CASES = sorted({c for v in CASES.values() for c in v})


@functools.lru_cache(maxsize=None)
def make_cloud(dtype, mask, classes, per_cell, box, signed=False):
    key = (dtype, mask, classes, per_cell, box) + (("signed",) if signed else ())
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    q, pairs = cu.cloud(box, RC, np.dtype(dtype), mask, classes, rng, per_cell=per_cell, with_pairs=True,
                        nonneg_open=mask not in (0, 7) and not signed)
    q.setflags(write=False)
    return q, pairs


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
def reference(dtype, mask, classes, per_cell, box, signed, full):
    """(counts[n], key_pointer[n + 1], list) of the cloud, per-row ascending.  Mask 0: oracle.build (full: symmetrised, the
    two differences being exact negatives in an open box); mask 7: build_pbc / build_pbc_full; a mixed mask: the padded
    reference of tests/test_periodic_axes.py, its open axes widened to 2 L + 2 rc first so that the particles up to a box
    length above the box still lie inside the padded box, unshifted; a signed mixed-mask cloud, whose negative open-axis
    coordinates that reference does not admit: cutoff_util.brute_force, which test_the_brute_force_is_the_oracles holds
    against the three references above."""
    from tests.test_periodic_axes import reference as padded_reference

    q = make_cloud(dtype, mask, classes, per_cell, box, signed)[0]
    po = _po()
    if signed:
        return brute_force_lists(dtype, mask, classes, per_cell, box, signed)[full]
    if mask == 0:
        h = po.build(q, RC, box)
        return _symmetrised(h.key_pointer, h.sorted_list) if full else _canonical(h.key_pointer, h.sorted_list)
    if mask == 7:
        h = (po.build_pbc_full if full else po.build_pbc)(q, RC, box)
    else:
        wide = tuple(box[d] if mask >> d & 1 else 2.0 * box[d] + 2.0 * RC for d in range(3))
        assert all(mask >> d & 1 or (q[:, d].min() >= 0 and q[:, d].max() < wide[d]) for d in range(3))
        h = padded_reference(q, RC, wide, mask, full=full)
    return _canonical(h.key_pointer, h.sorted_list)


@functools.lru_cache(maxsize=None)
def brute_force_lists(*c):
    """{full: (counts, key_pointer, list)} of a cloud by cutoff_util.brute_force."""
    cnt, kp, lst = cu.brute_force(make_cloud(*c)[0], c[4], RC, c[1])
    rows = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    up = lst > rows
    hcnt = np.bincount(rows[up], minlength=len(cnt))
    return {True: (cnt, kp, lst), False: (hcnt, np.concatenate([[0], np.cumsum(hcnt)]), lst[up])}


def mix_sum(row_ids, counts, lst):
    """The checksum of include/nl_hip.h (nl_list_checksum) in numpy: the wrapping sum of mix((id_i << 32) | j)."""
    v = (np.repeat(np.asarray(row_ids, dtype=np.uint64), counts) << np.uint64(32)) | np.asarray(lst, dtype=np.uint64)
    v = v * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    return int(v.sum(dtype=np.uint64))


def stencil_streams(q, box):
    """Particles of the 27 cells around every cell (periodic wrap), from the oracle's cell ids: [mz, my, mx]."""
    cell, m = _po().cells(np.ascontiguousarray(q), RC, box)
    assert np.all(cell >= 0)
    cnt = np.bincount(cell, minlength=int(m[0] * m[1] * m[2])).reshape(m[2], m[1], m[0])
    tot = np.zeros_like(cnt)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                tot += np.roll(cnt, (dz, dy, dx), axis=(0, 1, 2))
    return tot


# ------------------------------------------------------------------------------------------------------ CPU: the input


def wrapped_open_face(name, mask, signed):
    """A face class on an open axis of an unsigned mixed-mask cloud: every low-face partner is wrapped in, a box length away."""
    return name in cu.FACE and not mask >> cu.FACE[name] & 1 and mask not in (0, 7) and not signed


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: f"{c[0]}-m{c[1]}-{'+'.join(c[2])}-{c[3]:g}-{c[4][2]:.6f}{'-signed' if c[5] else ''}")
def test_the_clouds_sit_on_the_cutoff(c):
    """Per class: >= 25 constructed pairs accepted and >= 25 rejected within 16 ulp_T(rc2), r2 by the header's rule in the
    row that decides the pair (the smaller id).  Exempt is only the face class on the open axis of an unsigned mixed-mask
    cloud, where the padded reference forces three partners in four to be wrapped in, a box length away (they test that
    nothing is invented); the signed cloud of the same mask and class is held to the condition.  zplane: of the accepted near-cut-off pairs, >= 10 exactly 3 and
    >= 10 exactly 4 quarter-planes apart, upwards and downwards."""
    dtype, mask, classes, per_cell, box, signed = c
    q, pairs = make_cloud(*c)
    m = cu.mesh(box)
    assert q.dtype == np.dtype(dtype) and len(q) == int(round(per_cell * m[0] * m[1] * m[2]))
    rows, cols = np.minimum(pairs["a"], pairs["b"]), np.maximum(pairs["a"], pairs["b"])
    r2, visited = cu.rule_r2(q, rows, cols, box, RC, mask)
    acc = visited & ~(r2.astype(np.float64) > RC * RC)
    near = visited & cu.near_cutoff(r2, RC)
    for name in classes:
        sel = pairs["cls"] == name
        n_in, n_out = int((sel & near & acc).sum()), int((sel & near & ~acc).sum())
        print(f"{dtype} mask {mask} {name}: {n_in} accepted, {n_out} rejected within 16 ulp of rc2 ({int(sel.sum())} pairs)")
        if not wrapped_open_face(name, mask, signed):
            assert n_in >= 25 and n_out >= 25, (name, n_in, n_out)
        if name == "zplane":
            Q = cu.quarter_index(q, box, RC)
            up = q[pairs["b"], 2] > q[pairs["a"], 2]
            diff = np.abs(Q[pairs["a"]] - Q[pairs["b"]])
            for direction, dsel in (("up", up), ("down", ~up)):
                n3, n4 = (int((sel & near & acc & dsel & (diff == k)).sum()) for k in (3, 4))
                print(f"    {direction}: {n3} accepted pairs 3 quarter-planes apart, {n4} pairs 4 apart")
                assert n3 >= 10 and n4 >= 10, (direction, n3, n4)


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: f"{c[0]}-m{c[1]}-{'+'.join(c[2])}-{c[3]:g}-{c[4][2]:.6f}{'-signed' if c[5] else ''}")
def test_the_rule_is_the_oracles(c):
    """The numpy rule the self-check counts with decides every constructed pair as the oracle's list does, in both rows."""
    dtype, mask, classes, per_cell, box, signed = c
    q, pairs = make_cloud(*c)

    def listed(want, rows, cols):
        cnt, _, lst = want
        keys = (np.repeat(np.arange(len(cnt), dtype=np.int64), cnt) << 32) | lst
        return np.isin((rows.astype(np.int64) << 32) | cols, keys)

    for rows, cols in ((pairs["a"], pairs["b"]), (pairs["b"], pairs["a"])):
        want = cu.accepted(q, rows, cols, box, RC, mask)
        got = listed(reference(*c, True), rows, cols)
        assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], pairs["cls"][got != want][:8])
    rows, cols = np.minimum(pairs["a"], pairs["b"]), np.maximum(pairs["a"], pairs["b"])
    assert np.array_equal(listed(reference(*c, False), rows, cols), cu.accepted(q, rows, cols, box, RC, mask))


BRUTE_CHECKED = sorted(c for k, v in CASES.items() if k.startswith("masks-") for c in v if not c[5])


@pytest.mark.parametrize("c", BRUTE_CHECKED, ids=lambda c: f"{c[0]}-m{c[1]}-{'+'.join(c[2])}")
def test_the_brute_force_is_the_oracles(c):
    """cutoff_util.brute_force, the reference of the signed mixed-mask clouds, gives the oracle's list entry for entry on
    every cloud that has one: oracle.build (mask 0), build_pbc and build_pbc_full (mask 7), the padded reference (mask 5);
    half and full, fp32 and fp64."""
    for full in (False, True):
        got, want = brute_force_lists(*c)[full], reference(*c, full)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (c, full)


# ------------------------------------------------------------------------------------------------------ the device


def handle(box, n, dtype, mask, full):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(RC, *box, dtype=torch.float32 if dtype == F32 else torch.float64, full_list=full)  # (reads the environment)
    if mask:
        nl.set_periodic(axes=tuple(bool(mask >> d & 1) for d in range(3)))
    nl.Initialize(n)
    return nl


def assert_plan(nl, expect, what):
    info, stats = nl.build_info(), nl.build_stats()
    for name, want in expect.items():
        have = info[name] if name in info else stats[name]
        assert want(have) if callable(want) else have == want, (what, name, have, info, stats)


def assert_list(nl, want, what):
    cnt, kp, lst = want
    if nl.full_list:
        gkp, glst, gcnt = (t.cpu().numpy() for t in nl.full_csr())
    else:
        gkp, glst, gcnt = (t.cpu().numpy() for t in (nl.key_pointer(), nl.sorted_list(), nl.half_number_of_partners()))
    bad = np.flatnonzero(gcnt != cnt)
    assert not len(bad), (what, f"{len(bad)} rows differ; row {bad[0]}: {gcnt[bad[0]]} partners, the oracle {cnt[bad[0]]}", nl.build_info())
    assert np.array_equal(gkp.astype(np.int64), kp), what
    rows = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    key = (rows << 32) | glst.astype(np.int64)
    key.sort()
    glst = key & 0xFFFFFFFF
    if not np.array_equal(glst, lst):
        r = int(rows[np.flatnonzero(glst != lst)[0]])
        raise AssertionError((what, f"row {r}: got {glst[kp[r]:kp[r + 1]]}, the oracle {lst[kp[r]:kp[r + 1]]}", nl.build_info()))
    assert nl.list_checksum() == (mix_sum(np.arange(len(cnt)), cnt, lst), int(kp[-1])), what


def run_cases(name, expect, kinds=(False, True), builds=1, each=None):
    """Every cloud of CASES[name], half and full list: the path assertion first, then the list.  each(nl, q, box): further
    assertions on every handle after its last build."""
    torch = _torch()
    for c in CASES[name]:
        dtype, mask, classes, per_cell, box, signed = c
        q = make_cloud(*c)[0]
        qd = torch.from_numpy(np.array(q)).cuda()
        for full in kinds:
            nl = handle(box, len(q), dtype, mask, full)
            for _ in range(builds):
                nl.MakeNeighList(qd, len(q))
                assert_plan(nl, expect, (c, full))
                assert_list(nl, reference(*c, full), (c, full))
            if each is not None:
                each(nl, q, box)


@gpu
def test_lean_two_wave(monkeypatch):
    monkeypatch.setenv("NL_ROWS", "0")
    run_cases("lean", dict(masks=True, small_cells=1, fine_rows=0, mask_rows=1, variant=3))


BINNINGS = {"bucket": {}, "two_pass": {"NL_BIN_BUCKETS": "0"}, "atomic": {"NL_BINNING": "1"}}


@gpu
@pytest.mark.parametrize("binning", list(BINNINGS))
@pytest.mark.parametrize("mask", [0, 5, 7])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_four_wave_masks(dtype, mask, binning, monkeypatch):
    """The one-batch hit masks (k_sweep_lean_f32 with 4 waves / the screened fp64 search / the minimum-image instances)
    behind each of the three binnings: k_bin_bucket, k_bin_scatter and k_reorder each store a wrapped particle's image.
    Mask 5 also on the signed clouds: the minimum-image instances with negative coordinates on their open axis."""
    monkeypatch.setenv("NL_ROWS", "0")
    monkeypatch.setenv("NL_IDCLASS", "0")
    for k, v in BINNINGS[binning].items():
        monkeypatch.setenv(k, v)
    run_cases(f"masks-{dtype}-{mask}", dict(masks=True, small_cells=0, fine_rows=0, mask_rows=1, id_classes=0, binning=binning))


@gpu
@pytest.mark.parametrize("c", ["2", "4"])
def test_id_classes(c, monkeypatch):
    monkeypatch.setenv("NL_ROWS", "0")
    monkeypatch.setenv("NL_IDCLASS", c)
    run_cases("idclass", dict(masks=True, small_cells=0, fine_rows=0, id_classes=int(c)), kinds=(False,))


@gpu
@pytest.mark.parametrize("rows", ["1", "2", "3", "default"])
def test_fine_rows(rows, monkeypatch):
    """NL_ROWS = 1, 2, 3: RowsCfg<0..2> at 30 per cell; the default environment at 50 per cell."""
    if rows == "default":
        monkeypatch.delenv("NL_ROWS", raising=False)
        run_cases("rows-50", dict(masks=True, fine_rows=lambda v: v > 0))
    else:
        monkeypatch.setenv("NL_ROWS", rows)
        run_cases("rows-30", dict(masks=True, fine_rows=int(rows)))


@gpu
def test_fine_rows_overflow(monkeypatch):
    """A crowded cell whose stream exceeds RowsCfg<0>::CAP (read from nl_rows.hpp, so the condition follows the kernel) goes
    to k_rows_overflow, next to cells of the fine-row search.  The library reports no count of such cells; that the cell is
    beyond the buffer is asserted on the input, from the oracle's cells."""
    monkeypatch.setenv("NL_ROWS", "1")
    (c,) = CASES["rows-overflow"]
    assert stencil_streams(make_cloud(*c)[0], c[4]).max() > ROWS0_CAP
    run_cases("rows-overflow", dict(masks=True, fine_rows=1))


@gpu
@pytest.mark.parametrize("above", [True, False])
def test_fine_row_margin(above, monkeypatch):
    """ms_z / rc about 2^-30 above the threshold of rows_margin_ok: the fine rows run, and pairs 4 quarter-planes apart sit
    at the edge of their reach with no slack left; about 2^-30 below: the build must leave them out."""
    monkeypatch.setenv("NL_ROWS", "4")
    run_cases("margin-above" if above else "margin-below",
              dict(masks=True, fine_rows=(lambda v: v > 0) if above else 0))


@gpu
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_dense_masks(dtype, mask, monkeypatch):
    monkeypatch.setenv("NL_ROWS", "0")
    run_cases(f"dense-{dtype}-{mask}", dict(masks=True, mask_rows=lambda v: v > 1, fine_rows=0))


@gpu
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_two_sweeps(dtype, mask, monkeypatch):
    """NL_SWEEP_VARIANT=1: the COUNT and FILL distance sweeps decide every pair twice, and must decide it alike."""
    monkeypatch.setenv("NL_SWEEP_VARIANT", "1")
    run_cases(f"dense-{dtype}-{mask}", dict(variant=1, masks=False))


@gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_batched_list_kernels(dtype, monkeypatch):
    """A cell whose stencil stream exceeds the LDS batch the build reports: k_sweep_list_f32 / the batched sweep and
    k_fill_list take it, in their half and their full instances, also in the builds past the ones that launch them
    unconditionally (every handle must still report them launched after its last build)."""
    monkeypatch.setenv("NL_ROWS", "0")
    monkeypatch.setenv("NL_IDCLASS", "0")
    handles = []

    def launched(nl, q, box):
        assert stencil_streams(q, box).max() > nl.build_info()["lds_batch"] > 0, nl.build_info()
        assert nl.build_stats()["list_launched"], nl.build_stats()
        handles.append(nl.full_list)

    run_cases(f"list-{dtype}", dict(masks=True, small_cells=0, fine_rows=0, mask_rows=1), builds=LIST_QUIET_BUILDS + 2,
              each=launched)
    assert handles == [False, True]


@gpu
@pytest.mark.parametrize("mask", [0, 7])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_slabs(dtype, mask, monkeypatch):
    """The clouds as three z-slabs (5 layers: two box-end ranks and an interior one) on one device, identity ids carried
    as a gid array: a box-end rank forms the z image while it bins the ghost layer, the whole build in the search; the
    union of the rows is the whole-box reference entry for entry and the checksums add up to its checksum.
    Regression (float32, mask 7, face_z, slab [0, 2)): a lower ghost with z < 0, wrapped into the top layer and standing for
    layer -1, was stored at z itself, where a whole build takes it at rn(rn(z + L) - L): one partner of one row differed."""
    from md_neighbor_list_amd import slab
    from tests.test_slab_paths import make_handle, run_decomposition, slab_parts

    monkeypatch.setenv("NL_ROWS", "0")
    layers = slab.split_layers(cu.mesh(BOX)[2], 3)
    assert layers == [(0, 2), (2, 4), (4, 5)]
    for c in CASES[f"slab-{dtype}-{mask}"]:
        q = make_cloud(*c)[0]
        parts = slab_parts(q, BOX, RC, layers, mask)
        assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(len(q)))
        for full in (False, True):
            nl = make_handle(BOX, max(len(p["order"]) for p in parts), np.dtype(dtype), mask=mask, full=full)
            run_decomposition(nl, q, parts, reference(*c, full), (c, full),
                              expect=dict(masks=True, small_cells=0, fine_rows=0, mask_rows=1))

"""nl_update_list on every build path: the gated build against the oracle, skipped updates byte for byte.

An update's build is a chain of gated launches behind k_skin_check: every kernel of it must leave at entry while the `go`
word is 0 and must produce exactly nl_make_list's list while it is 1.  Each case here drives one handle along one
five-step trajectory (below) on one search path / binning / offset width, and

  after an update that built   compares counts, key_pointer, per-row ascending partners, the entry counts and the
                               checksum with the oracle's list of those positions (list_of of tests/test_slab_paths.py:
                               the oracle alone, never a second run of the library), and asserts through build_info() /
                               build_stats() that the case's path was the one taken;
  after an update that skipped compares key_pointer (both widths of a wide build), the list, the counts, the cell table
                               and sorted_row of sorted_state(), the checksum, build_info() and build_stats() byte for
                               byte with what was read after the last build.

Three ways: every update synchronous with the checks after each step; the five updates enqueued on one stream without
a host wait; the same chain replayed from a graph (nl_set_graph).  Every comparison is exact: integers, bytes, checksums.

The trajectory (skin s = 0.6, h = s / 2; positions in the handle's type, clipped to [0, L)):
  q0  make_input(...)                                                    u(q0) builds (forced)
  q1  q0 + a random displacement of at most 0.45 h for every particle;
      one interior particle p moves exactly +0.6 h in x instead          u(q1) skips
  q2  q0                                                                 u(q2) skips
  q3  q1 with p at q0_p + 1.1 h in x: 0.5 h from the previous positions,
      1.1 h from the snapshot -- a skipped update that had taken a
      snapshot would not build here                                      u(q3) builds
  q4  q3 + displacements of at most 0.45 h for every particle            u(q4) skips
The expected decisions come from a numpy replay of rule (c) of include/nl_hip.h, per axis of the mask.  The CPU test shows
that the skip checks have teeth: q1 and q4 have other lists and other cells than q0 and q3, so any stage of a build that
ran on a skipped update's positions would change an array compared here.

Boxes and densities are those of tests/test_slab_paths.py; D = 3 x 3 x 3 cells at 340 particles per cell (mean stencil
stream 9180, with 5 sigma + 64 7.6 LDS batches: more than FD_NB = 7) is where plan_build's default variant falls back
to the two sweeps, in plain builds as well.
"""
import functools
import itertools
import zlib

import numpy as np
import pytest

from tests.test_slab_paths import (BOXES, FORCED, RC, ROWS_CAP, expected_plan, list_of, make_handle, make_input, mesh, mix_sum,
                                   read_slab, stencil_streams)

SKIN = 0.6
H = 0.5 * SKIN
DECISIONS = (True, False, False, True, False)  # what the recipe is made for; the tests take them from replay()
LDS_BATCH = 1280  # nl_kernels.hpp: SweepCfg::CAP, read back as build_info()["lds_batch"]
gpu = pytest.mark.gpu


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


# ------------------------------------------------------------------------------------------------------ trajectory


def _jiggled(q, rng, box):
    """q + a random displacement of length at most 0.45 h per particle, in q's type, clipped to [0, L)."""
    dt = q.dtype.type
    step = rng.normal(size=(len(q), 3))
    step *= (0.45 * H * rng.random((len(q), 1))) / np.linalg.norm(step, axis=1, keepdims=True)
    hi = np.array([np.nextafter(dt(b), dt(0)) for b in box], dtype=q.dtype)
    out = q.copy()
    out[:, :3] = np.clip(q[:, :3] + step.astype(q.dtype), dt(0), hi)
    return out


@functools.lru_cache(maxsize=None)
def trajectory(key):
    """((q0 .. q4), p) of the module docstring for the input make_input(*key); read-only, the same for every mask."""
    q0, box = make_input(*key), BOXES[key[0]]
    dt = q0.dtype.type
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    inner = np.all((q0[:, :3] > 1.0) & (q0[:, :3] < np.array(box) - 1.0), axis=1)
    p = int(np.flatnonzero(inner)[0])
    q1 = _jiggled(q0, rng, box)
    q1[p, :3] = q0[p, :3]
    q1[p, 0] = q0[p, 0] + dt(0.6 * H)
    q3 = q1.copy()
    q3[p, 0] = q0[p, 0] + dt(1.1 * H)
    q4 = _jiggled(q3, rng, box)
    seq = (q0, q1, q0, q3, q4)
    for q in seq:
        q.setflags(write=False)
    return seq, p


def r2_of(q, snap, box, mask):
    """Rule (c) of include/nl_hip.h: d in the position type, widened to double; folded with rint on the axes of the mask
    only; (dx^2 + dy^2) + dz^2 without FMA."""
    d = (q[:, :3] - snap[:, :3]).astype(np.float64)  # (numpy subtracts in the arrays' type, rounded to nearest)
    for a in range(3):
        if mask >> a & 1:
            L = np.float64(box[a])
            d[:, a] = d[:, a] - L * np.rint(d[:, a] / L)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def replay(seq, box, mask):
    """(built[k], snap[k]) per step: does update k build, and the step whose positions the list holds after it."""
    thr = (0.5 * SKIN) ** 2
    built, snaps, snap = [True], [0], 0
    for k in range(1, len(seq)):
        r2 = r2_of(seq[k], seq[snap], box, mask)
        b = bool(np.isnan(r2).any() or r2.max() > thr)
        snap = k if b else snap
        built.append(b)
        snaps.append(snap)
    return tuple(built), tuple(snaps)


@functools.lru_cache(maxsize=40)
def want(key, mask, full, step):
    """(counts, key_pointer, per-row ascending partners, checksum of nl_hip.h) of trajectory(key)'s step: the oracle's."""
    cnt, kp, lst = list_of(trajectory(key)[0][step], BOXES[key[0]], mask, full)
    return cnt, kp, lst.astype(np.int32), mix_sum(np.arange(len(cnt)), cnt, lst)


def whole(q, box):
    """The whole box as one slab, for stencil_streams."""
    return dict(order=np.arange(len(q)), z_lo=0, z_hi=mesh(box)[2])


# ------------------------------------------------------------------------------------------------------ the cases
# (environment, input key, mask, what build_info() / build_stats() must say, list kinds, stream bound or None)


def _case(env, key, mask, expect, kinds=("half", "full"), over=None):
    name = "-".join([f"{k}={v}" for k, v in env.items()] + [key[0] + str(key[1]), key[2][-2:]] +
                    ([key[3] + str(key[4])] if key[3] != "uniform" else []) + [f"m{mask}"])
    return dict(env=env, key=key, mask=mask, expect=expect, kinds=kinds, over=over, name=name)


def _uniform(box, per_cell, dtype):
    return (box, per_cell, dtype, "uniform", 0)


DEFAULT = [_case({}, _uniform(b, d, t), m, dict(expected_plan(d, t, m), variant=3, offset_bits=32))
           for b in "AB" for d, masks in ((8, (0, 7)), (30, (0, 7, 3)), (50, (0, 7, 4)), (90, (0, 7, 3)))
           for t in ("float32", "float64") for m in masks]

# the rows of FORCED (tests/test_slab_paths.py) an update has a path for, with the same expectations
_FORCED_ROWS = {("NL_ROWS", "1", 30), ("NL_ROWS", "2", 30), ("NL_ROWS", "3", 30), ("NL_ROWS", "1", 50), ("NL_ROWS", "0", 50),
                ("NL_SWEEP_VARIANT", "1", 30), ("NL_SWEEP_VARIANT", "1", 50), ("NL_BINNING", "1", 30), ("NL_BINNING", "1", 50),
                ("NL_OFFSET_WIDTH", "64", 30), ("NL_OFFSET_WIDTH", "64", 50)}
_picked = [f for f in FORCED if (*next(iter(f[0].items())), f[1]) in _FORCED_ROWS]
assert len(_picked) == len(_FORCED_ROWS)
PATHS = [_case(env, _uniform("B", d, t), m, dict(expect, **({"id_classes": 0} if "NL_BINNING" in env else {})),
               over=ROWS_CAP[1] if env == {"NL_ROWS": "1"} and d == 50 else None)  # (streams beyond RowsCfg<0>: k_rows_overflow)
         for env, d, dtypes, masks, expect in _picked for t in dtypes for m in masks]
# the id-class search (half list only); "0": the plain one-batch search of the fp32 open box, which NL_IDCLASS's default hides
PATHS += [_case({"NL_IDCLASS": c}, _uniform("B", 30, "float32"), 0, dict(id_classes=int(c), masks=True, mask_rows=1, fine_rows=0),
                kinds=("half",)) for c in ("2", "4", "0")]

CROWDS = [  # the update's own build hands cells to the batched kernels (k_sweep_list_f32 / k_fill_list, k_rows_overflow)
    _case({}, ("C", 8, "float32", "crowd", 1300), 0, dict(small_cells=1, masks=True, mask_rows=1, fine_rows=0), over="lds_batch"),
    _case({}, ("C", 25, "float64", "crowd", 1300), 0, dict(small_cells=0, masks=True, mask_rows=1), over="lds_batch"),
    _case({}, ("C", 25, "float64", "crowd", 1300), 7, dict(small_cells=0, masks=True, mask_rows=1), over="lds_batch"),
    _case({}, ("C", 8, "float32", "block", 60), 0, dict(small_cells=1, masks=True, mask_rows=1, fine_rows=0), over="lds_batch"),
    _case({"NL_ROWS": "4"}, ("B", 50, "float32", "crowd", 1700), 0, dict(fine_rows=lambda v: v > 0), over="rows"),
]

BEYOND = [_case({}, _uniform("D", 340, t), m, dict(variant=3, masks=False, fine_rows=0)) for t in ("float32", "float64") for m in (0, 7)]

CASES = DEFAULT + PATHS + CROWDS
WAYS = ("sync", "async", "graph")


def _ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------------ CPU


def test_trajectory_decisions_and_teeth_on_the_cpu():
    """For every input and mask of this file: the replay of rule (c) builds at exactly steps 0 and 3, and would not build
    at step 3 from a snapshot of q1; the positions lie in [0, L); q1 / q4 have another list than q0 / q3 (in the counts,
    and in the partners of rows whose counts agree) and another cell for some particle, so that a stage which ran on a
    skipped update's positions shows in the arrays the GPU tests compare.  The crowd inputs hold a 27-cell stream
    beyond the LDS batch (the fine-row cases: beyond the buffer of their RowsCfg)."""
    po = _po()
    thr = (0.5 * SKIN) ** 2
    seen = set()
    for c in CASES + BEYOND:
        key, mask = c["key"], c["mask"]
        if (key, mask) in seen:
            continue
        seen.add((key, mask))
        box = BOXES[key[0]]
        seq, p = trajectory(key)
        for q in seq:
            assert q.dtype == np.dtype(key[2]) and np.all(q[:, :3] >= 0) and np.all(q[:, :3] < np.array(box)), key
        built, snaps = replay(seq, box, mask)
        assert built == DECISIONS and snaps == (0, 0, 0, 3, 3), (key, mask, built)
        assert r2_of(seq[3], seq[1], box, mask).max() <= thr, (key, mask)  # (a snapshot of q1 would have kept the list)
        assert np.flatnonzero(r2_of(seq[3], seq[0], box, mask) > thr).tolist() == [p], (key, mask)  # (p alone decides the build at q3)
        for a, b in ((0, 1), (3, 4)):
            ca, _, la = list_of(seq[a], box, mask, False)
            cb, kb, lb = list_of(seq[b], box, mask, False)
            same = np.flatnonzero((ca == cb) & (ca > 0))
            assert (ca != cb).any(), (key, mask, a, b)  # the counts differ
            ka = np.concatenate([[0], np.cumsum(ca)])
            # and so do the partners of rows with equal counts
            assert any(not np.array_equal(la[ka[r]:ka[r + 1]], lb[kb[r]:kb[r + 1]]) for r in same), (key, mask, a, b)
            cell_a, cell_b = po.cells(seq[a], RC, box)[0], po.cells(seq[b], RC, box)[0]
            assert np.all(cell_a >= 0) and np.all(cell_b >= 0) and (cell_a != cell_b).any(), (key, mask, a, b)
    for c in CASES:
        if c["over"] is not None:
            q0, box = trajectory(c["key"])[0][0], BOXES[c["key"][0]]
            bound = {"lds_batch": LDS_BATCH, "rows": max(ROWS_CAP.values())}.get(c["over"], c["over"])
            assert stencil_streams(q0, whole(q0, box), box).max() > bound, c["name"]
    q0 = trajectory(BEYOND[0]["key"])[0][0]
    assert len(q0) == 9180 and stencil_streams(q0, whole(q0, BOXES["D"]), BOXES["D"]).min() == 9180  # (27 cells: every stream is the box)


# ------------------------------------------------------------------------------------------------------ GPU helpers


def check_list(nl, key, mask, step, what, wide=False):
    """The handle's list == the oracle's list of trajectory(key)'s step.  Returns read_slab's dict."""
    got = read_slab(nl, wide)
    cnt, kp, lst, cs = want(key, mask, nl.full_list, step)
    bad = np.flatnonzero(got["counts"] != cnt)
    assert not len(bad), (f"{what}: row {bad[0]} has {got['counts'][bad[0]]} partners, the oracle {cnt[bad[0]]} at step {step}; "
                          f"{len(bad)} rows differ; {got['info']}")
    assert np.array_equal(got["key_pointer"], kp), what
    if not np.array_equal(got["partners"], lst):
        k = int(np.flatnonzero(got["partners"] != lst)[0])
        r = int(np.searchsorted(kp, k, side="right") - 1)
        raise AssertionError(f"{what}: row {r} at step {step}: got {got['partners'][kp[r]:kp[r + 1]]}, the oracle "
                             f"{lst[kp[r]:kp[r + 1]]}; {got['info']}")
    total = int(kp[-1])
    assert got["entries"] == total and got["checksum_entries"] == total, (what, got["entries"], total)
    assert got["half_pairs"] == (total // 2 if nl.full_list else total), what
    assert got["checksum"] == cs, what
    return got


def check_path(got, case, what, q0=None):
    """build_info() / build_stats() say that the case's path was taken, by an update's build."""
    info, stats = got["info"], got["stats"]
    for name, w in case["expect"].items():
        have = info[name] if name in info else stats[name]
        assert w(have) if callable(w) else have == w, (what, name, have, info, stats)
    assert stats["cap_row"] == 0 and stats["list_launched"], (what, stats)  # (two-pass or atomic binning, every launch)
    if case["over"] is not None and q0 is not None:
        bound = {"lds_batch": info["lds_batch"], "rows": ROWS_CAP.get(info["fine_rows"], 0)}.get(case["over"], case["over"])
        assert bound > 0 and stencil_streams(q0, whole(q0, BOXES[case["key"][0]]), BOXES[case["key"][0]]).max() > bound, (what, bound)
        if case["over"] == "lds_batch":
            assert bound == LDS_BATCH, (what, info)


def raw_state(nl, wide):
    """Everything a skipped update must leave as it is, as bytes and plain values."""
    if nl.full_list:
        kp, lst, cnt = nl.full_csr(32)
        kp64 = nl.full_csr(64)[0] if wide else None
    else:
        kp, lst, cnt = nl.key_pointer(), nl.sorted_list(), nl.half_number_of_partners()
        kp64 = nl.key_pointer64() if wide else None
    cs, sr = nl.sorted_state()
    out = {name: t.cpu().numpy().tobytes() for name, t in (("key_pointer", kp), ("list", lst), ("counts", cnt), ("cell_start", cs),
                                                           ("sorted_row", sr), ("key_pointer64", kp64)) if t is not None}
    out.update(checksum=nl.list_checksum(), info=nl.build_info(), stats=nl.build_stats(), entries=nl.list_entries())
    return out


def same_state(a, b, what):
    assert a.keys() == b.keys(), what
    for name in a:
        assert a[name] == b[name], f"{what}: a skipped update changed {name}"


def capacity_for(case):
    """Entries an asynchronous handle needs for every build of the case's trajectory."""
    return max(int(want(case["key"], case["mask"], kind == "full", step)[1][-1]) for kind in case["kinds"] for step in (0, 3))


def run_sync(nl, case, kind, stats, wide):
    """Way 1: every update waits; the checks of the module docstring after each step."""
    torch = _torch()
    key, mask = case["key"], case["mask"]
    seq = trajectory(key)[0]
    built, snaps = replay(seq, BOXES[key[0]], mask)
    qd = torch.from_numpy(np.array(seq[0])).cuda()
    last = None
    for k in range(len(seq)):
        what = (case["name"], kind, "sync", k)
        if k:
            qd.copy_(torch.from_numpy(np.array(seq[k])))
        nl.update(qd, sync=True)
        stats[0], stats[1] = stats[0] + 1, stats[1] + int(built[k])
        assert nl.update_stats() == tuple(stats), (what, nl.update_stats(), stats)
        for w in ((True, False) if wide else (False,)):
            got = check_list(nl, key, mask, snaps[k], what, wide=w)  # (after a skip: still the snapshot's list)
        if built[k]:
            check_path(got, case, what, q0=seq[0] if k == 0 else None)
            last = raw_state(nl, wide)
        else:
            same_state(last, raw_state(nl, wide), what)


def run_enqueued(nl, case, kind, stats, wide, graph):
    """Ways 2 and 3: the five updates on one stream without a host wait (way 3: the forced one plain, the next captured,
    three replayed), one synchronize(); then, way 3, one more synchronous update, which skips."""
    torch = _torch()
    key, mask = case["key"], case["mask"]
    seq = trajectory(key)[0]
    built, snaps = replay(seq, BOXES[key[0]], mask)
    what = (case["name"], kind, "graph" if graph else "async")
    dev = torch.from_numpy(np.stack(seq)).cuda()  # every position set up front
    qd = dev[0].clone()
    nl.update(qd)
    for k in range(1, len(seq)):
        qd.copy_(dev[k], non_blocking=True)
        nl.update(qd)
    nl.synchronize()
    stats[0], stats[1] = stats[0] + len(seq), stats[1] + sum(built)
    assert nl.update_stats() == tuple(stats), (what, nl.update_stats(), stats)
    for w in ((True, False) if wide else (False,)):
        got = check_list(nl, key, mask, snaps[-1], what, wide=w)
    check_path(got, case, what)
    if graph:
        before = raw_state(nl, wide)
        nl.update(qd, sync=True)  # q4 again: replayed, skips
        stats[0] += 1
        assert nl.update_stats() == tuple(stats), (what, nl.update_stats(), stats)
        same_state(before, raw_state(nl, wide), what)
        check_list(nl, key, mask, snaps[-1], what)


def run_case(case, way, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)  # (read when the handle is created)
    key, mask = case["key"], case["mask"]
    wide = case["env"].get("NL_OFFSET_WIDTH") == "64"
    n = len(trajectory(key)[0][0])
    nl = make_handle(BOXES[key[0]], n, key[2], mask, graph=way == "graph", capacity=None if way == "sync" else capacity_for(case))
    nl.set_skin(SKIN)
    stats = [0, 0]
    for kind in case["kinds"]:
        nl.set_full_list(kind == "full")  # (forces the next update's build, as the first update of a handle is forced)
        if way == "sync":
            run_sync(nl, case, kind, stats, wide)
        else:
            run_enqueued(nl, case, kind, stats, wide, way == "graph")


# ------------------------------------------------------------------------------------------------------ GPU


@gpu
@pytest.mark.parametrize("case,way", list(itertools.product(CASES, WAYS)), ids=[f"{c['name']}-{w}" for c, w in itertools.product(CASES, WAYS)])
def test_update_on_every_path(case, way, monkeypatch):
    """The default plan at 8, 30, 50 and 90 particles per cell in boxes A and B; the forced paths (fine rows and their
    overflow kernel, dense masks, two sweeps, atomic binning, 64-bit offsets read through both getters, id classes);
    boxes with a crowd.  Half and full list on one handle, three ways."""
    run_case(case, way, monkeypatch)


@gpu
@pytest.mark.parametrize("case", BEYOND, ids=_ids(BEYOND))
def test_beyond_seven_batches(case, monkeypatch):
    """Box D at 340 per cell: streams of more than FD_NB LDS batches, where the default variant falls back to two
    sweeps.  A plain build, synchronous and asynchronous, half and full, against the oracle; then the synchronous
    update sequence on another handle."""
    torch = _torch()
    key, mask = case["key"], case["mask"]
    q0, box = trajectory(key)[0][0], BOXES[key[0]]
    nl = make_handle(box, len(q0), key[2], mask, capacity=capacity_for(case))
    qd = torch.from_numpy(np.array(q0)).cuda()
    for kind in case["kinds"]:
        nl.set_full_list(kind == "full")
        for sync in (True, False):
            nl.MakeNeighList(qd, len(q0), sync=sync)
            if not sync:
                nl.synchronize()
            what = (case["name"], kind, "plain", sync)
            got = check_list(nl, key, mask, 0, what)
            for name, w in case["expect"].items():
                assert got["info"][name] == w, (what, name, got["info"])
    del nl
    run_case(case, "sync", monkeypatch)


REFILL = [  # one case per FILL family of finish()'s refill after growth: box B, mask 0
    _case({}, _uniform("B", 8, "float32"), 0, dict(small_cells=1, masks=True, mask_rows=1, fine_rows=0)),
    _case({}, _uniform("B", 30, "float32"), 0, dict(small_cells=0, masks=True, mask_rows=1, fine_rows=0)),  # (half: the id-class expansion)
    _case({}, _uniform("B", 30, "float64"), 0, dict(small_cells=0, masks=True, mask_rows=1, fine_rows=0)),
    _case({}, _uniform("B", 90, "float32"), 0, dict(masks=True, mask_rows=3, fine_rows=0)),
    _case({}, _uniform("B", 50, "float32"), 0, dict(fine_rows=2)),
    _case({"NL_SWEEP_VARIANT": "1"}, _uniform("B", 30, "float32"), 0, dict(variant=1, masks=False, fine_rows=0)),
    _case({"NL_OFFSET_WIDTH": "64"}, _uniform("B", 30, "float32"), 0, dict(offset_bits=64, masks=True)),
]


@gpu
@pytest.mark.parametrize("kind", ["half", "full"])
@pytest.mark.parametrize("case", REFILL, ids=_ids(REFILL))
def test_capacity_refill_per_fill_family(case, kind, monkeypatch):
    """E = the oracle's entry count of q0.  A capacity of E holds an asynchronous update without growth.  With E - 1 the
    asynchronous update fails at synchronize(), the next one builds and fails again, the synchronous one grows the list
    and refills it with the ungated FILL of the build's plan; the update after it skips and leaves every byte."""
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    key, mask, full = case["key"], case["mask"], kind == "full"
    wide = case["env"].get("NL_OFFSET_WIDTH") == "64"
    seq = trajectory(key)[0]
    box, n = BOXES[key[0]], len(seq[0])
    E = int(want(key, mask, full, 0)[1][-1])
    qd = torch.from_numpy(np.array(seq[0])).cuda()

    nl = make_handle(box, n, key[2], mask, full=full, capacity=E)
    nl.set_skin(SKIN)
    nl.update(qd)
    nl.synchronize()
    assert nl.update_stats() == (1, 1)
    check_path(check_list(nl, key, mask, 0, (case["name"], kind, "E")), case, (case["name"], kind, "E"))

    nl = make_handle(box, n, key[2], mask, full=full, capacity=E - 1)
    nl.set_skin(SKIN)
    for k in (1, 2):
        nl.update(qd)
        with pytest.raises(NLError) as e:
            nl.synchronize()
        assert e.value.code == NL_ERR_CAPACITY, (case["name"], kind, k)
        assert nl.update_stats() == (k, k)  # (the host has seen the failure: the second one builds, and fails, again)
    nl.update(qd, sync=True)  # grows the list and refills it
    assert nl.update_stats() == (3, 3)
    what = (case["name"], kind, "E - 1")
    for w in ((True, False) if wide else (False,)):
        got = check_list(nl, key, mask, 0, what, wide=w)
    check_path(got, case, what)
    before = raw_state(nl, wide)
    qd.copy_(torch.from_numpy(np.array(seq[1])))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (4, 3)
    same_state(before, raw_state(nl, wide), what)
    check_list(nl, key, mask, 0, what)

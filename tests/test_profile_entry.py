"""The profiling entry points (nl_profile_last_build, nl_profile_stages): the list and the state they leave behind.

They are not passive timers.  nl_profile_last_build plans the last build again as one whole build (plan_for(..., PART_ALL,
the last plan's rerun)), runs it `reps` times on the handle's own stream into the handle's live buffers, from the positions the
caller's buffer holds NOW, adopts it and finishes it: the list, the counts, the plan, build_info() and build_stats()
afterwards are that build's.  Every stage time the project has published went through these two calls, so:

  1. after profiling, the list is still the oracle's list of the caller's positions -- on every search path, binning,
     offset width and list kind of tests/test_update_paths.py, with every feature that adds a stage or a buffer, after a
     slab build (one call, begin / finish, local ids) and, in tests/dist_paths_worker.py, on one rank of a distributed
     build -- build_info() is what it was, and the next build is exact as well;
  2. the seven numbers are finite, not negative, and the six stages add up to the total within a bound derived below
     (test_stage_times_add_up); the error codes are those of include/nl_hip.h;
  3. a profiled build between two updates is "a build other than an update's": the next nl_update_list builds (rule (a) of
     include/nl_hip.h), so that no pair can come inside the physical cut-off unseen.

Expectations come from the oracle alone (list_of / global_list of tests/test_slab_paths.py, want of
tests/test_update_paths.py; the rule replay of tests/test_triclinic_box.py for the tilted box, the numpy filters of
tests/test_exclusions.py and tests/test_type_cutoffs.py, the float64 images of tests/test_pair_images.py), never from a
second run of the library.  Every list comparison is exact.  reps = 2 everywhere, but for one case at reps = 1.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests.test_slab_paths import (BOXES, DECOMPS, LIST_QUIET_BUILDS, RC, build_slab, check_rows, global_list, list_of, make_handle,
                                   make_input, mesh, mix_sum, read_slab, relabelled, slab_parts, stencil_streams)
from tests.test_update_paths import CASES, CROWDS, want
from tests.util import canonical_csr

gpu = pytest.mark.gpu
STAGES = ("hash", "cell_scan", "reorder", "count", "row_scan", "fill", "total")
KEY = ("B", 30, "float32", "uniform", 0)  # the feature handles: box B = 5 x 4 x 6 cells, 30 per cell, fp32


def _torch():
    import torch

    return torch


def _device(q):
    return _torch().from_numpy(np.array(q)).cuda()


# ------------------------------------------------------------------------------------------------------ helpers


def expectation(cnt, kp, lst):
    """(counts, key_pointer, per-row ascending partners, checksum of nl_hip.h) of a canonical CSR: the form of want()."""
    cnt, kp = np.asarray(cnt, dtype=np.int64), np.asarray(kp, dtype=np.int64)
    return cnt, kp, np.asarray(lst), mix_sum(np.arange(len(cnt)), cnt, lst)


def read_list(nl, wide=False):
    """(key_pointer, list, counts) of the last build on the host, through the getters of the handle's list kind."""
    if nl.full_list:
        kp, lst, cnt = nl.full_csr(64 if wide else 32)
    else:
        kp, lst, cnt = (nl.key_pointer64() if wide else nl.key_pointer()), nl.sorted_list(), nl.half_number_of_partners()
    return kp.cpu().numpy().astype(np.int64), lst.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)


def check_oracle(nl, expect, what, wide=False):
    """The handle's list == expect: counts, key_pointer (both widths of a wide build), every row after the canonical
    sort, the entry counts and the checksum."""
    cnt, kp, lst, cs = expect
    for w in ((True, False) if wide else (False,)):
        got_kp, got_lst, got_cnt = read_list(nl, w)
        bad = np.flatnonzero(got_cnt != cnt) if len(got_cnt) == len(cnt) else np.array([-1])
        assert not len(bad), f"{what}: row {bad[0]} differs in its count; {len(bad)} rows differ; {nl.build_info()}"
        assert np.array_equal(got_kp, kp), what
        assert np.array_equal(canonical_csr(got_kp, got_lst), lst), what
    total = int(kp[-1])
    assert nl.list_entries() == total, (what, nl.list_entries(), total)
    assert nl.half_number_of_pairs() == (total // 2 if nl.full_list else total), what
    assert nl.list_checksum() == (cs, total), what


def check_times(ms, what):
    """All seven values, finite and not negative; the search stages and the total took some time."""
    assert tuple(ms) == STAGES, (what, tuple(ms))
    assert all(math.isfinite(v) and v >= 0.0 for v in ms.values()), (what, ms)
    assert ms["total"] > 0.0 and ms["count"] > 0.0 and ms["fill"] > 0.0, (what, ms)


def around_profile(nl, check, what, reps=2, same_info=True):
    """check("before"), profile_last_build, check("after"); build_info() is the recorded one in every field."""
    check(f"{what}: before profiling")
    info = nl.build_info()
    ms = nl.profile_last_build(reps=reps)
    check_times(ms, what)
    check(f"{what}: after profiling")
    if same_info:
        assert nl.build_info() == info, (what, info, nl.build_info())
    return ms


def rebuild_async(nl, qd, n):
    nl.MakeNeighList(qd, n, sync=False)
    nl.synchronize()


# ------------------------------------------------------------------------------------------------------ 1. every path

PATH_CASES = [c for c in CASES if c["key"][0] == "B" or any(c is k for k in CROWDS)]
DEFAULT_HALF = ({}, KEY, 0)  # the case that must run the id-class search with the reach cull


@gpu
@pytest.mark.parametrize("case", PATH_CASES, ids=[c["name"] for c in PATH_CASES])
def test_list_survives_profiling_on_every_path(case, monkeypatch):
    """Every case of tests/test_update_paths.py on box B and its five crowded boxes, half and full list where the case has
    both: MakeNeighList(sync=True), the oracle's list; profile_last_build; the oracle's list and the same build_info();
    an asynchronous build; the oracle's list."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)  # (read when the handle is created)
    key, mask = case["key"], case["mask"]
    wide = case["env"].get("NL_OFFSET_WIDTH") == "64"
    q, box = make_input(*key), BOXES[key[0]]
    default_half = (case["env"], key, mask) == DEFAULT_HALF
    # (an asynchronous build cannot grow its list)
    nl = make_handle(box, len(q), key[2], mask, capacity=max(int(want(key, mask, kind == "full", 0)[1][-1]) for kind in case["kinds"]))
    qd = _device(q)
    for kind in case["kinds"]:
        nl.set_full_list(kind == "full")
        expect = want(key, mask, kind == "full", 0)
        what = (case["name"], kind)

        def check(stage):
            check_oracle(nl, expect, (what, stage), wide)
            if default_half and kind == "half":
                info = nl.build_info()
                assert info["id_classes"] == 2 and info["reach_cull"], (what, stage, info)

        nl.MakeNeighList(qd, len(q), sync=True)
        info = nl.build_info()
        for name, w in case["expect"].items():  # the case's path is the one a plain build takes as well
            if name in info:
                assert w(info[name]) if callable(w) else info[name] == w, (what, name, info)
        around_profile(nl, check, what, reps=1 if default_half and kind == "half" else 2)
        rebuild_async(nl, qd, len(q))
        check("the next build")


# ------------------------------------------------------------------------------------------------------ 1. features


def _input():
    return make_input(*KEY), BOXES["B"]


@gpu
def test_profiling_a_tilted_box():
    """set_box with a tilt (xy = 0.2 Lx, mask 7): 4 x 4 x 6 sheared cells; the expectation is the rule replay."""
    from tests import test_triclinic_box as tri

    box6 = BOXES["B"] + (0.2 * BOXES["B"][0], 0.0, 0.0)
    assert tri.mesh_of(RC, box6) == (4, 4, 6)
    q = tri.positions(len(make_input(*KEY)), RC, box6, 7, np.float32, seed=5)
    kp, lst = tri.replay(q, RC, box6, 7, np.float32)
    expect = expectation(np.diff(kp), kp, lst)
    nl = make_handle(BOXES["B"], len(q), "float32", 7, capacity=int(kp[-1]))
    nl.set_box(*box6)
    qd = _device(q)
    nl.MakeNeighList(qd, len(q), sync=True)
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "tilt")
    rebuild_async(nl, qd, len(q))
    check_oracle(nl, expect, "tilt: the next build")


@gpu
def test_profiling_with_exclusions():
    """A few hundred excluded pairs taken from the oracle's list: the profiled build runs the filter stage, and the list,
    nl_number_of_pairs and the checksum are the filtered ones before and after."""
    from tests.test_exclusions import remove_pairs

    q, box = _input()
    cnt, kp, lst = global_list(KEY, 0, False)
    rows = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    pick = np.arange(0, len(lst), len(lst) // 300)
    pairs = np.stack([rows[pick], lst[pick]], axis=1).astype(np.int32)
    assert 300 <= len(pairs) <= 400
    expect = expectation(*remove_pairs(kp, lst, pairs))
    assert expect[1][-1] == kp[-1] - len(pairs)
    nl = make_handle(box, len(q), "float32", capacity=int(kp[-1]))  # (the capacity counts the list before the filter)
    nl.set_exclusions(pairs, len(q))
    qd = _device(q)
    nl.MakeNeighList(qd, len(q), sync=True)
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "exclusions")
    rebuild_async(nl, qd, len(q))
    check_oracle(nl, expect, "exclusions: the next build")


@gpu
def test_profiling_with_type_cutoffs():
    """Two types with unequal cut-offs: the expectation is the oracle's list through the numpy type filter."""
    from tests.test_type_cutoffs import _want

    q, box = _input()
    types = (np.arange(len(q)) % 3 == 0).astype(np.int32)
    rcm = np.array([[RC, 0.8 * RC], [0.8 * RC, 0.9 * RC]])
    expect = expectation(*_want(q, RC, box, 0, False, np.float32, types, rcm))
    assert 0 < expect[1][-1] < global_list(KEY, 0, False)[1][-1]
    nl = make_handle(box, len(q), "float32", capacity=int(global_list(KEY, 0, False)[1][-1]))
    nl.set_type_cutoffs(types, rcm)
    qd = _device(q)
    nl.MakeNeighList(qd, len(q), sync=True)
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "types")
    rebuild_async(nl, qd, len(q))
    check_oracle(nl, expect, "types: the next build")


def _images_by_row(nl):
    """(rows, partners, images) of the last build with every row sorted by partner."""
    ei = nl.edge_index().cpu().numpy()
    img = nl.pair_images().cpu().numpy()
    assert img.shape == (nl.list_entries(), 3), (img.shape, nl.list_entries())
    order = np.argsort((ei[0] << 32) | ei[1], kind="stable")
    return ei[0][order], ei[1][order], img[order].astype(np.int64)


@gpu
def test_profiling_with_pair_images():
    """nl_set_pair_images on a periodic box: the profiled build runs the image stage; pair_images() has list_entries()
    rows, equals the float64 reference and the images from before, row by row."""
    from tests.test_pair_images import image_ref

    q, box = _input()
    expect = expectation(*list_of(q, box, 7, False))
    nl = make_handle(box, len(q), "float32", 7, capacity=int(expect[1][-1]))
    nl.set_pair_images(True)
    qd = _device(q)
    seen = []

    def check(stage):
        check_oracle(nl, expect, stage)
        rows, parts, img = _images_by_row(nl)
        assert np.array_equal(parts, expect[2]), stage  # (rows sorted by partner: the canonical list)
        assert np.array_equal(img, image_ref(q, box + (0.0, 0.0, 0.0), 7, rows, parts)[0]), stage
        assert (img != 0).any(axis=1).mean() > 0.05, stage  # (entries across a periodic face)
        seen.append(img)

    nl.MakeNeighList(qd, len(q), sync=True)
    around_profile(nl, check, "images")
    rebuild_async(nl, qd, len(q))
    check("images: the next build")
    assert all(np.array_equal(seen[0], s) for s in seen[1:])


def _check_transposed(nl, expect, what):
    """neigh_list() / number_of_partners() are a transpose of the CSR the handle returns, which is the oracle's."""
    check_oracle(nl, expect, what)
    n = len(expect[0])
    t = nl.neigh_list().cpu().numpy()
    cnt = nl.number_of_partners().cpu().numpy()
    assert np.array_equal(cnt[:n], expect[0]), what
    assert t.shape[0] >= int(expect[0].max()), what
    got = np.concatenate([np.sort(t[:cnt[i], i]) for i in range(n)])
    assert np.array_equal(got, expect[2]), what


@gpu
def test_profiling_a_full_list_read_transposed():
    """A full list fetched as neigh_list() before and after.  Then the caller's positions change in place and the profiler
    builds from them: the transposed form fetched afterwards is the transpose of THAT list, not the one made before."""
    from tests.test_update_paths import trajectory

    seq, _p = trajectory(KEY)
    box = BOXES["B"]
    e0, e1 = want(KEY, 0, True, 0), want(KEY, 0, True, 1)
    assert not np.array_equal(e0[0], e1[0])  # (another list)
    nl = make_handle(box, len(seq[0]), "float32", full=True, capacity=max(int(e0[1][-1]), int(e1[1][-1])))
    qd = _device(seq[0])
    nl.MakeNeighList(qd, len(seq[0]), sync=True)
    around_profile(nl, lambda s: _check_transposed(nl, e0, s), "transposed")
    qd.copy_(_torch().from_numpy(np.array(seq[1])))
    check_times(nl.profile_last_build(reps=2), "transposed, moved")
    _check_transposed(nl, e1, "transposed: after profiling moved positions")
    rebuild_async(nl, qd, len(seq[0]))
    _check_transposed(nl, e1, "transposed: the next build")


@gpu
def test_profiling_between_graph_replays(monkeypatch):
    """NL_GRAPH=1: a captured and a replayed build, the profiler's plain launches, two more replays -- all exact."""
    monkeypatch.setenv("NL_GRAPH", "1")
    q, box = _input()
    expect = want(KEY, 0, False, 0)
    nl = make_handle(box, len(q), "float32", capacity=int(expect[1][-1]))
    qd = _device(q)
    for k in range(2):
        rebuild_async(nl, qd, len(q))
        check_oracle(nl, expect, f"graph: build {k}")
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "graph")
    for k in range(2, 4):
        rebuild_async(nl, qd, len(q))
        check_oracle(nl, expect, f"graph: build {k}")


@gpu
def test_profiling_a_list_that_was_grown():
    """set_capacity(1000), then a synchronous build that grows the list and refills it: the profiler runs in the grown list."""
    q, box = _input()
    expect = want(KEY, 0, False, 0)
    assert expect[1][-1] > 1000
    nl = make_handle(box, len(q), "float32", capacity=1000)
    qd = _device(q)
    nl.MakeNeighList(qd, len(q), sync=True)
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "grown")
    rebuild_async(nl, qd, len(q))
    check_oracle(nl, expect, "grown: the next build")


@gpu
def test_profiling_after_the_crowd_arrives():
    """LIST_QUIET_BUILDS + 1 quiet builds, after which the handle leaves the launches for cells beyond the LDS buffer out;
    then a crowd (streams beyond the buffer), then the profiler.  Whether the profiled build launches those kernels or is
    run again by finish(): the list is the oracle's."""
    crowd = ("B", 30, "float32", "crowd", 1000)  # (4600 particles: still the one-batch mask search)
    q0, q1, box = make_input(*KEY), make_input(*crowd), BOXES["B"]
    e0, e1 = expectation(*global_list(KEY, 0, False)), expectation(*global_list(crowd, 0, False))
    whole = dict(order=np.arange(len(q1)), z_lo=0, z_hi=mesh(box)[2])
    nl = make_handle(box, len(q1), "float32", capacity=int(e1[1][-1]))
    assert stencil_streams(q1, whole, box).max() > nl.build_info()["lds_batch"] > 0
    d0, d1 = _device(q0), _device(q1)
    for _ in range(LIST_QUIET_BUILDS + 1):
        nl.MakeNeighList(d0, len(q0), sync=True)
    check_oracle(nl, e0, "quiet")
    assert not nl.build_stats()["list_launched"], nl.build_stats()
    nl.MakeNeighList(d1, len(q1), sync=True)
    info = nl.build_info()
    assert info["masks"] and info["mask_rows"] == 1 and info["fine_rows"] == 0, info  # (the path with those launches)
    around_profile(nl, lambda s: check_oracle(nl, e1, s), "crowd", same_info=False)
    rebuild_async(nl, d1, len(q1))
    check_oracle(nl, e1, "crowd: the next build")
    nl.MakeNeighList(d0, len(q0), sync=True)
    around_profile(nl, lambda s: check_oracle(nl, e0, s), "quiet again", same_info=False)


# ------------------------------------------------------------------------------------------------------ 1. slab builds


@gpu
@pytest.mark.parametrize("how", ["one_call", "begin_finish", "local_ids"])
def test_profiling_a_slab_build(how):
    """The middle part of a 3-way split of box B, as tests/test_slab_paths.py builds it on one GPU: the rows take_rows cuts
    from the global list before and after; nl_number_of_pairs and the checksum unchanged.  (The profiler runs a begin /
    finish pair as one whole build.)"""
    q, box = _input()
    part = slab_parts(q, box, RC, DECOMPS["B2"][1])[1]
    glob, ids = global_list(KEY, 0, False), None
    nl = make_handle(box, len(part["order"]), "float32")
    if how == "local_ids":
        # ids are rows of the slab's buffer: owned first, ghosts behind them (particles the slab does not hold: beyond)
        nl.set_local_ids(True)
        ids = np.full(len(q), -1, dtype=np.int64)
        ids[part["order"]] = np.arange(len(part["order"]))
        ids[ids < 0] = len(part["order"]) + np.arange(int((ids < 0).sum()))
        glob = relabelled(glob, ids, False)
        qa = _device(q[part["order"]])
        nl.MakeNeighListSlab(qa, None, len(part["own"]), part["z_lo"], part["z_hi"], sync=True)
        got = read_slab(nl)
    else:
        got = build_slab(nl, q, part, split=how == "begin_finish")
    cs = check_rows(got, part, glob, (how, "before"), ids=ids)
    ms = nl.profile_last_build(reps=2)
    check_times(ms, how)
    after = read_slab(nl)
    assert check_rows(after, part, glob, (how, "after"), ids=ids) == cs == after["checksum"]
    assert after["half_pairs"] == got["half_pairs"] and after["entries"] == got["entries"], how


# ------------------------------------------------------------------------------------------------------ 2. the numbers

# What hipEventElapsedTime documents for its result: "a resolution of around 0.5 microseconds".
EVENT_RESOLUTION_MS = 0.5e-3


def sum_bound(total_ms):
    """The bound of test_stage_times_add_up for a total of total_ms milliseconds."""
    return 7 * (2.0 ** -24 * total_ms + 2 * EVENT_RESOLUTION_MS)


@gpu
@pytest.mark.parametrize("env,binning", [({}, "bucket"), ({"NL_BIN_BUCKETS": "0"}, "two_pass"), ({"NL_BINNING": "1"}, "atomic")])
def test_stage_times_add_up(env, binning, monkeypatch):
    """Every binning records its own events (a path that never recorded one would hand hipEventElapsedTime a stale or an
    unrecorded event).  All 7 values are finite and >= 0; total, count and fill are > 0; total == the sum of the 6 stages
    within sum_bound(total).

    The bound.  The 7 events e0 .. e6 of a build lie on one stream; stage k is elapsed(e_k, e_k+1), the total
    elapsed(e0, e6).  In exact arithmetic the six differences telescope to the total.  Each of the 7 values reaches the
    caller as a float32 number of milliseconds, within 2^-24 relative of itself and so within 2^-24 total each (no
    stage exceeds the total): 7 x 2^-24 total.  Each value is a difference of two time stamps that the runtime reads with
    the documented resolution r = 0.5 us, so it is off by at most 2 r should the two ends be rounded independently:
    7 x 2 r.  The averages over `reps` builds are sums of such values in double (exact at this size) over reps, so they
    keep the bound: |total - sum| <= 7 (2^-24 total + 2 r) = 7e-3 ms + 4.2e-7 total.  Nothing is asserted about how large
    a time is."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    q, box = _input()
    expect = want(KEY, 0, False, 0)
    nl = make_handle(box, len(q), "float32")
    qd = _device(q)
    nl.MakeNeighList(qd, len(q), sync=True)
    assert nl.build_info()["binning"] == binning, nl.build_info()
    ms = around_profile(nl, lambda s: check_oracle(nl, expect, s), binning)
    assert nl.build_info()["binning"] == binning
    diff = abs(ms["total"] - sum(ms[k] for k in STAGES[:6]))
    print(f"{binning}: total {ms['total']:.6f} ms, |total - sum of stages| = {diff:.3e} ms, bound {sum_bound(ms['total']):.3e} ms")
    assert diff <= sum_bound(ms["total"]), (binning, ms, diff, sum_bound(ms["total"]))


@gpu
def test_profile_stages_builds_and_profiles():
    """profile_stages(q, reps) on a handle that has only been initialised: the same keys, the oracle's list of q, and the
    particle count the getters need."""
    q, box = _input()
    expect = want(KEY, 0, False, 0)
    nl = make_handle(box, len(q), "float32")
    ms = nl.profile_stages(_device(q), reps=2)
    check_times(ms, "profile_stages")
    assert nl._n == nl._n_rows == len(q)
    check_oracle(nl, expect, "profile_stages")


@gpu
def test_profile_errors():
    """Through the C ABI: NL_ERR_STATE before any build; NL_ERR_ARG for reps <= 0 and a null result; NL_ERR_CAPACITY, and
    nothing run, after an asynchronous build that overflowed its list -- a synchronous build then grows it and profiling
    works."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_CAPACITY, NL_ERR_STATE, NL_NUM_STAGES, NLError

    q, box = _input()
    expect = want(KEY, 0, False, 0)
    nl = make_handle(box, len(q), "float32", capacity=1000)
    lib, h = nl._lib, nl._h
    ms = (C.c_double * NL_NUM_STAGES)(*([-1.0] * NL_NUM_STAGES))
    assert lib.nl_profile_last_build(h, 2, C.byref(ms)) == NL_ERR_STATE  # (no build yet)
    for reps in (0, -1):
        assert lib.nl_profile_last_build(h, reps, C.byref(ms)) == NL_ERR_ARG
    assert lib.nl_profile_last_build(h, 2, None) == NL_ERR_ARG
    qd = _device(q)
    assert lib.nl_profile_stages(h, qd.data_ptr(), 4, len(q), 0, C.byref(ms)) == NL_ERR_ARG
    assert lib.nl_profile_stages(h, qd.data_ptr(), 4, len(q), 2, None) == NL_ERR_ARG
    assert list(ms) == [-1.0] * NL_NUM_STAGES
    nl.MakeNeighList(qd, len(q), sync=False)  # overflows the 1000 entries
    assert lib.nl_profile_last_build(h, 2, C.byref(ms)) == NL_ERR_CAPACITY
    assert list(ms) == [-1.0] * NL_NUM_STAGES  # (nothing was run: not even the result cleared)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    nl.MakeNeighList(qd, len(q), sync=True)  # grows the list
    around_profile(nl, lambda s: check_oracle(nl, expect, s), "after growth")


# ------------------------------------------------------------------------------------------------------ 3. between updates

SKIN = 0.4
CUT = RC - SKIN  # the physical cut-off: 2.9
HALF_SEP = {0: 1.55, 1: 1.73, 2: 1.37}  # A - B separation / 2 at P0, P1, P2: 3.10, 3.46, 2.74 (each moves 0.18 = 0.45 skin)
CLEAR = 0.5  # no other particle within this of A or B


def skin_scenario():
    """((P0, P1, P2), a, b): box B at 8 per cell, fp32, open, plus particles A and B (rows a, b) on a line along x through
    the middle of a row of x-cells -- the first such row, from the middle of the box outwards, around which the uniform
    particles leave them CLEAR -- at the separations of HALF_SEP.  No other particle moves."""
    base, box = make_input("B", 8, "float32"), BOXES["B"]
    m = mesh(box)
    ms = [b / k for b, k in zip(box, m)]
    rows = sorted(itertools.product(range(m[1]), range(m[2])), key=lambda r: (abs(r[0] + 0.5 - m[1] / 2) + abs(r[1] + 0.5 - m[2] / 2), r))
    for cy, cz in rows:
        y, z, x = (cy + 0.5) * ms[1], (cz + 0.5) * ms[2], 0.5 * box[0]
        spots = np.array([[x + s * h, y, z] for h in HALF_SEP.values() for s in (-1.0, 1.0)])
        d = np.linalg.norm(base[None, :, :3].astype(np.float64) - spots[:, None, :], axis=2)
        if d.min() > CLEAR + 0.01:
            break
    else:
        raise AssertionError("no clear row")
    seq = []
    for step in (0, 1, 2):
        ab = np.zeros((2, 4), dtype=np.float32)
        ab[:, :3] = [[x - HALF_SEP[step], y, z], [x + HALF_SEP[step], y, z]]
        seq.append(np.concatenate([base, ab]))
    return tuple(seq), len(base), len(base) + 1


def has_pair(cnt, kp, lst, a, b):
    return int(b) in lst[kp[a]:kp[a + 1]].tolist()


def test_the_skin_scenario_is_what_it_claims():
    """From the oracle and numpy alone: both moves stay below skin / 2 for every particle (rule (c) skips), the oracle's
    list lacks the pair (A, B) at P1 and has it at P0 and P2, and at P2 the two are inside the physical cut-off."""
    from tests.test_update_paths import r2_of

    (p0, p1, p2), a, b = skin_scenario()
    box = BOXES["B"]
    for p in (p0, p1, p2):
        assert p.dtype == np.float32 and np.all(p[:, :3] >= 0) and np.all(p[:, :3] < np.array(box))
        others = np.delete(p[:, :3].astype(np.float64), (a, b), axis=0)
        for k in (a, b):
            assert np.linalg.norm(others - p[k, :3].astype(np.float64), axis=1).min() > CLEAR
    for p in (p1, p2):
        move = np.linalg.norm((p[:, :3] - p0[:, :3]).astype(np.float64), axis=1)
        assert move.max() <= 0.19 and np.flatnonzero(move > 0).tolist() == [a, b]
        assert move[[a, b]].min() > 0.17
        assert r2_of(p, p0, box, 0).max() <= (0.5 * SKIN) ** 2  # rule (c) of include/nl_hip.h keeps the list
    sep = [float(np.linalg.norm(p[a, :3].astype(np.float64) - p[b, :3].astype(np.float64))) for p in (p0, p1, p2)]
    assert abs(sep[0] - 3.10) < 1e-5 and abs(sep[1] - 3.46) < 1e-5 and abs(sep[2] - 2.74) < 1e-5
    assert sep[2] < CUT < sep[0] < RC < sep[1]
    assert has_pair(*list_of(p0, box, 0, False), a, b)
    assert not has_pair(*list_of(p1, box, 0, False), a, b)
    assert has_pair(*list_of(p2, box, 0, False), a, b)


@gpu
@pytest.mark.parametrize("way", ["last_build", "last_build_graph", "stages"])
def test_a_profiled_build_between_updates_forces_the_next_one(way, monkeypatch):
    """update(P0) builds; update(P1) skips (0.45 skin from P0) and keeps the list of P0; the profiler builds the list of P1,
    which lacks (A, B); update(P2) -- 0.45 skin from P0, 0.9 skin from P1 -- must build by rule (a) of include/nl_hip.h: a
    build other than an update's ran since.  Had it skipped against the snapshot of P0, A and B would be 2.74 apart,
    inside the physical cut-off of 2.9, and in no list.  On the commit before this test, update_stats() here was (3, 1)
    after nl_profile_last_build (plain and NL_GRAPH=1) and (3, 2) after nl_profile_stages, which builds through
    nl_make_list."""
    if way == "last_build_graph":
        monkeypatch.setenv("NL_GRAPH", "1")
    torch = _torch()
    seq, a, b = skin_scenario()
    box = BOXES["B"]
    lists = [list_of(p, box, 0, False) for p in seq]
    expect = [expectation(*g) for g in lists]
    nl = make_handle(box, len(seq[0]), "float32", capacity=max(int(e[1][-1]) for e in expect) + 64)
    nl.set_skin(SKIN)
    qd = _device(seq[0])

    def listed():
        kp, lst, cnt = read_list(nl)
        return has_pair(cnt, kp, lst, a, b)

    nl.update(qd, sync=True)
    assert nl.update_stats() == (1, 1)
    check_oracle(nl, expect[0], (way, "update(P0)"))
    qd.copy_(torch.from_numpy(seq[1]))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 1)
    check_oracle(nl, expect[0], (way, "update(P1) skipped"))
    assert listed()
    info = nl.build_info()
    ms = nl.profile_stages(qd, reps=2) if way == "stages" else nl.profile_last_build(reps=2)
    check_times(ms, way)
    if way != "stages":  # (planned as the update's build was: two passes of binning, every launch)
        assert nl.build_info() == info and info["binning"] == "two_pass", (way, info, nl.build_info())
    check_oracle(nl, expect[1], (way, "profiled at P1"))
    assert not listed()
    qd.copy_(torch.from_numpy(seq[2]))
    nl.update(qd, sync=True)
    stats = nl.update_stats()
    assert stats == (3, 2), f"{way}: update(P2) after a profiled build: update_stats() == {stats}, pair listed: {listed()}"
    check_oracle(nl, expect[2], (way, "update(P2)"))
    assert listed()
    nl.update(qd, sync=True)  # and the snapshot is P2's: the same positions again skip
    assert nl.update_stats() == (4, 2)
    check_oracle(nl, expect[2], (way, "update(P2) again"))

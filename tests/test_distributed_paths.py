"""Distributed builds (nl_make_list_distributed) per rank: every search path, periodic mask and capacity edge.

The one build path whose kernels do not know their particle count when launched: the host sizes the launches for
n_upper = owned + the two message capacities (clipped to the rows there are), the ghost counts are read on the device,
the search path is chosen from an estimate.  At a few hundred particles per rank the 1024-particle floor of a message
capacity makes n_upper several times the true count: the smallest shapes are the hardest for kernels that bound
themselves by a device-side count.

Every rank checks ITS rows: row r must equal row gid_owned[r] of the oracle's list of the undivided box (check_rows of
tests/test_slab_paths.py: counts, key_pointer, ascending partners, entries, nl_number_of_pairs, nl_list_checksum), its
ghost counts the populations of its two neighbour layers, its layers slab.split_layers.  Bit for bit, no tolerance.  Every
configuration is built twice, synchronously and asynchronously.  Each GPU test is one spawn (tests/dist_paths_worker.py)
that loops over its configurations; no world is above 5.

Boxes at rc = 3.3: A = 3 x 3 x 7 cells, B = 5 x 4 x 6, C = 5 x 5 x 8, D = 3 x 3 x 3, E = 3 x 3 x 4.
"""
import numpy as np
import pytest

from md_neighbor_list_amd import slab
from tests.dist_paths_worker import (F32, TESTS, Caps, crowd_extra, first_build_plan, get_input, get_list, halo_capacity, layers_of,
                                     lists_of_case, list_sum, parts_of, run)
from tests.test_slab_paths import BOXES, expected_plan, list_of, mesh, mix_sum, take_rows

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ CPU


def emulated_rows(q, box, part, mask, full):
    """The rows of one rank from the oracle on q[own ++ glo ++ ghi] and the ownership rule: (row ids, partners), sorted.
    Half list: a pair sits in the row of its smaller global id, on the rank that owns that particle."""
    order, n_rows = part["order"], len(part["own"])
    cnt, _, lst = list_of(np.ascontiguousarray(q[order]), box, mask, full)
    a = np.repeat(np.arange(len(order), dtype=np.int64), cnt)
    ga, gb = order[a], order[lst]
    if full:
        keep = a < n_rows
        rows, vals = ga[keep], gb[keep]
    else:
        keep = np.where(ga < gb, a, lst) < n_rows
        rows, vals = np.minimum(ga, gb)[keep], np.maximum(ga, gb)[keep]
    srt = np.lexsort((vals, rows))
    return rows[srt], vals[srt]


def test_rank_expectations_on_the_cpu():
    """The expectations themselves, without the library: for every (box, world, input, mask, list kind) of the GPU tests the
    rows emulated per rank are the rows take_rows cuts from the global list, every entry appears exactly once over the
    ranks, and the ranks' checksums add up to the global one.  Also what the GPU tests assume of their inputs: the search
    path expected_plan names is the one each rank's own estimate gives, the inputs with particles below z = 0 are filed
    differently with and without the periodic z, the crowd outgrows a message, the move changes every rank's counts."""
    seen = set()
    for name, (world, _env, cases) in TESTS.items():
        for case in cases:
            for key, mask, full in lists_of_case(case):
                if (world, key, mask, full) in seen:
                    continue
                seen.add((world, key, mask, full))
                q, box = get_input(key), BOXES[key[0]]
                glob = get_list(key, mask, full)
                assert glob[1][-1] > 0, (name, key)
                parts = parts_of(key, mask, world)
                assert [(p["z_lo"], p["z_hi"]) for p in parts] == slab.split_layers(mesh(box)[2], world)
                assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(len(q))), (name, key)
                entries, total = [], 0
                for p in parts:
                    rows, vals = emulated_rows(q, box, p, mask, full)
                    want_c, want_l = take_rows(glob, p["own"])
                    assert np.array_equal(np.bincount(np.searchsorted(p["own"], rows), minlength=len(p["own"])), want_c), (name, key, mask, full, p["z_lo"])
                    assert np.array_equal(vals, want_l), (name, key, mask, full, p["z_lo"])
                    entries.append((rows << 32) | vals)
                    total = (total + mix_sum(p["own"], want_c, want_l)) & (2**64 - 1)
                entries = np.concatenate(entries)
                assert len(np.unique(entries)) == len(entries) == glob[1][-1], (name, key, mask, full)
                assert total == list_sum(key, mask, full), (name, key, mask, full)
            if case["scenario"] == "plain":
                key, mask = case["key"], case["mask"]
                two_level = case.get("two_level", True)
                plan = expected_plan(30 if key[3] == "edges" else key[1], key[2], mask)
                for p in parts_of(key, mask, world):
                    assert first_build_plan(p, BOXES[key[0]], key[2], mask, two_level=two_level) == plan, (name, key, mask, p["z_lo"])
                if case.get("below"):
                    q, box = get_input(key), BOXES[key[0]]
                    assert (layers_of(q, box, mask) != layers_of(q, box, 0)).any(), (name, key, mask)
    # the open box and the minimum image give different, non-empty lists on the small boxes
    for box_name, per_cell in (("D", 8), ("E", 30), ("A", 8)):
        key = (box_name, per_cell, F32, "uniform", 0)
        assert 0 < get_list(key, 0, False)[1][-1] < get_list(key, 7, False)[1][-1], key
    # the crowd: a layer at the cut outgrows the capacity negotiated for the uniform part
    for dt in ("float32", "float64"):
        uni, crowd = parts_of(("C", 8, dt, "uniform", 0), 0, 2), parts_of(("C", 8, dt, "crowd", crowd_extra(dt)), 0, 2)
        assert len(crowd[0]["ghi"]) > halo_capacity(len(uni[0]["ghi"])) or len(crowd[1]["glo"]) > halo_capacity(len(uni[1]["glo"]))
    # the vacated layer is rank 2's only one; after the move every rank's owned and ghost counts differ and no layer has
    # outgrown a message (the capacities of round 0 stay: what the worker's estimate of n_est assumes)
    for dt in ("float32", "float64"):
        for mask in (0, 7):
            p0 = parts_of(("A", 30, dt, "vacated", 0), mask, 5)
            p1 = parts_of(("A", 30, dt, "moved", ("vacated", 0)), mask, 5)
            assert len(p0[2]["own"]) == 0 < len(p1[2]["own"]) and len(p0[1]["ghi"]) == 0 == len(p0[3]["glo"])
            for a, b in zip(p0, p1):
                assert len(a["own"]) != len(b["own"]) and (len(a["glo"]), len(a["ghi"])) != (len(b["glo"]), len(b["ghi"]))
                caps = Caps()
                caps.n_est(len(a["own"]), len(a["glo"]), len(a["ghi"]), 1 << 30)
                neg = list(caps.neg)
                caps.n_est(len(b["own"]), len(b["glo"]), len(b["ghi"]), 1 << 30)
                assert caps.neg == neg


# ------------------------------------------------------------------------------------------------------ GPU


def _run(name):
    world, env, cases = TESTS[name]
    res = run(world, cases, env=env)
    assert res[0] == "ok" and res[1] == len(cases)
    return res


@gpu
def test_one_layer_per_rank():
    """World 3 on the 3-layer box D: mzl = 3, a rank's one layer is its bottom and its top layer, and k_pack_layers appends
    every owned particle to both messages; both ghost layers are whole ranks.  8 and 50 per cell, fp32 and fp64, masks 0
    and 7, half and full list."""
    _run("one_layer")


@gpu
def test_two_ranks_share_both_ghost_layers():
    """World 2 on the 4-layer box E: both ghost layers of a rank are the peer's two layers (lo_peer == hi_peer: the order of
    the messages matters).  Uniform inputs; particles up to 0.9 box lengths outside (masks 0, 7); particles just outside
    every face under the mixed masks 3 and 4 against the padded reference.  With z periodic a particle below z = 0 belongs
    to the top rank: DistributedNeighList.scatter files by the library's own rule."""
    _run("two_ranks")


@gpu
def test_search_paths_under_device_side_counts():
    """World 3 on box A (3 + 2 + 2 layers) at 8, 30, 50 and 90 per cell: the small-cell path, one-batch masks, fine rows and
    dense mask rows, each asserted through build_info(), with n_upper unclipped (several times the true count at 8 per
    cell)."""
    _run("search_paths")


@gpu
def test_uneven_ranks_an_empty_rank_and_moving_particles():
    """World 5 on box A (2 + 2 + 1 + 1 + 1): layer 4 vacated, so rank 2 owns nothing (no pack launch; headers and build
    still run) and its neighbours' rows stay exact; then every particle moves, the same handles and communicators are
    scattered anew, and rank 2 owns particles."""
    _run("empty_rank")


@gpu
def test_rows_capacity_boundary_and_recovery():
    """World 2 on box B: rows for exactly owned + ghosts (n_upper clipped to the true total) build; one row fewer on rank
    0 is NL_ERR_CAPACITY there (HALO_ROWS_OVERFLOW: at the call, or at synchronize of an asynchronous build; ghost counts
    0 and 0) while rank 1 builds exactly; the same handle and communicator then build again with the right room."""
    _run("rows_boundary")


@gpu
def test_message_renegotiation_wide_elements_and_handle_changes():
    """World 2 on box C, one communicator per rank throughout: a crowd outgrows the capacities negotiated for the uniform
    part (NL_ERR_CAPACITY at synchronize, the next build renegotiates); a second, fp32 handle on the same communicator
    (16-byte elements after 32-byte ones) while the first keeps its rows; the same handle after every particle has moved;
    the communicator destroyed while both handles live.

    Left out: nl_set_graph(1) on a distributed build.  Its one run here (fp32 handle, three asynchronous builds with
    identical arguments) built exactly while the graph was captured and ended the first REPLAY with NL_ERR_HIP at
    nl_synchronize on both ranks; the cause is not found, so the configuration is not run again until it is."""
    _run("renegotiation")


@gpu
@pytest.mark.parametrize("name", ["host_counted", "host_counted_crowd"])
def test_host_counted_path(name):
    """NL_BINNING=1: no two-level binning, so the ghost counts are read back and nl_make_list_slab runs with them (world 3
    on box B); with the crowd on box C (world 2) the capacity flags travel through that branch and a synchronous build
    renegotiates."""
    _run(name)


@gpu
def test_profiling_one_rank_of_a_distributed_build():
    """World 2 on box A: after a synchronous and an asynchronous build rank 0 alone calls profile_last_build (what bench.py
    does at world > 1), which plans and runs the build again with the ghost counts on the device; both ranks' rows, ghost
    counts and checksums are still the oracle's, and so are those of the next collective build."""
    _run("profiled_rank")

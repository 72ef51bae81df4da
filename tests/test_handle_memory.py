"""The handle owns its device memory (md_neighbor_list_amd/csrc/nl_devbuf.hpp): what a handle allocated comes back when it
goes, a captured graph never replays a buffer that was replaced, and an allocation that fails leaves the handle usable.

All three on 4096 particles in fp32 in a box of 6 cells a side, against one oracle list (pyoracle.build) computed once.
"""
import gc

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.test_exclusions import _checksum, mixed_pairs, remove_pairs
from tests.util import canonical_csr

N = 4096
RC = 3.3
BOX = (20.0, 20.0, 20.0)  # int(20 / 3.3) = 6 cells a side
N_BIG = 2_000_000
CYCLES = 8


@pytest.fixture(scope="module")
def system():
    """(q, the oracle's canonical half list of it): shared by the tests, never written."""
    from oracle import pyoracle as po

    q, _ = inputs.uniform_box(N, dtype=np.float32, seed=15, box=BOX)
    ref = po.build(q, RC, BOX).canonical()
    for a in (q, ref.key_pointer, ref.sorted_list):
        a.setflags(write=False)
    return q, ref


def _assert_list(nl, ref, pairs, what):
    """The handle's half list is the oracle's without `pairs`: counts, offsets, canonical list, pair count, checksum."""
    counts, kp_w, lst_w = remove_pairs(ref.key_pointer, ref.sorted_list, pairs)
    kp = nl.key_pointer().cpu().numpy().astype(np.int64)
    lst = nl.sorted_list().cpu().numpy()
    assert np.array_equal(nl.half_number_of_partners().cpu().numpy(), counts), what
    assert np.array_equal(kp, kp_w), what
    assert np.array_equal(canonical_csr(kp, lst), lst_w), what
    assert nl.half_number_of_pairs() == len(lst_w), what
    assert nl.list_checksum() == (_checksum(kp_w, lst_w), len(lst_w)), what


NO_PAIRS = np.zeros((0, 2), dtype=np.int32)


def _cycle(torch, qd, ref, pairs_small, pairs_large, first):
    """One handle sized for N_BIG particles, every feature that owns device buffers switched on in turn on builds of N,
    then dropped.  Returns the free memory its first nl_initialize took (the handle's footprint).  first: check lists too."""
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(RC, *BOX, dtype=torch.float32)
    # (the list's capacity fixed first: the default follows n_max^2 / volume, 196 GB for N_BIG particles in this box)
    nl.set_capacity(4 * ref.npairs)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    nl.Initialize(N_BIG)  # per-particle buffers of several hundred MB; no build of that size
    torch.cuda.synchronize()
    footprint = before - torch.cuda.mem_get_info()[0]
    # exclusions: a table, a larger one in its place, a global one
    nl.set_exclusions(pairs_small, N)
    nl.MakeNeighList(qd, N)
    nl.set_exclusions(pairs_large, N)
    nl.MakeNeighList(qd, N)
    nl.resort(qd.clone())  # (the first re-sort after a build relabels the table: its scratch)
    nl.set_exclusions_global(pairs_large, N + 1000)
    nl.MakeNeighList(qd, N)
    if first:
        _assert_list(nl, ref, pairs_large, "global table")
    # type cut-offs (the typed stage, with the exclusions in it) and the typed consumer's parameters
    two = np.full((2, 2), RC)
    nl.set_type_cutoffs(torch.arange(N, dtype=torch.int32, device=qd.device) % 2, two)
    nl.set_lj_type_params(np.ones((2, 2)), np.ones((2, 2)), np.full((2, 2), 2.5))
    nl.MakeNeighList(qd, N)
    nl.lj_forces_typed(qd)
    nl.resort(qd.clone())  # (... and the types: equal cut-offs, so the lists below do not depend on them)
    # pair images on, then off
    nl.set_pair_images(True)
    nl.MakeNeighList(qd, N)
    assert nl.pair_images().shape[0] == nl.list_entries()
    nl.set_pair_images(False)
    # the skin snapshot
    nl.set_skin(0.3)
    nl.update(qd, N, sync=True)
    nl.update(qd, N, sync=True)
    nl.clear_type_cutoffs()
    nl.clear_exclusions()
    # a full list and its transposed form
    nl.set_full_list(True)
    nl.MakeNeighList(qd, N)
    assert nl.neigh_list().shape[1] == N
    nl.set_full_list(False)
    nl.MakeNeighList(qd, N)
    if first:
        _assert_list(nl, ref, NO_PAIRS, "plain build")
    kp32 = nl.key_pointer()
    assert torch.equal(nl.key_pointer64(), kp32.to(torch.int64))  # (the 64-bit getter after a 32-bit build: a converted copy)
    del kp32
    nl.resort(qd.clone())
    nl.set_box(24.0, 24.0, 24.0)  # 7 cells a side: the per-cell and per-row buffers grow
    nl.MakeNeighList(qd, N)
    assert nl.half_number_of_pairs() == ref.npairs  # (an open box: the same pairs in the larger one)
    nl.Initialize(N_BIG)
    nl.MakeNeighList(qd, N)
    assert nl.half_number_of_pairs() == ref.npairs
    del nl
    gc.collect()
    return footprint


@pytest.mark.gpu
def test_memory_comes_back(system):
    """CYCLES handles of several hundred MB, created, used with every buffer-owning feature and dropped: the device has
    as much free memory afterwards as before, to within half of one handle's footprint (one handle's main buffers leaked
    every other cycle would take 4 footprints; other tenants' allocations of a few MB do not matter).  Free memory by
    torch.cuda.mem_get_info: the device's, whoever allocated.  Measured (profiles/r15_devbuf.txt), before and after the
    handle's buffers became DevBufs alike: footprint 512 MiB, -36 MiB after the first cycle (code objects, pools) and after
    every later one."""
    import torch

    q, ref = system
    qd = torch.tensor(q).cuda()  # (a copy: q is read-only)
    pairs_small = mixed_pairs(ref.key_pointer, ref.sorted_list, N, 1, k=500)
    pairs_large = mixed_pairs(ref.key_pointer, ref.sorted_list, N, 2, k=20000)
    torch.cuda.synchronize()
    start = torch.cuda.mem_get_info()[0]
    trace, footprint = [], None
    for k in range(CYCLES):
        fp = _cycle(torch, qd, ref, pairs_small, pairs_large, k == 0)
        footprint = footprint or fp  # (of the first nl_initialize)
        torch.cuda.synchronize()
        trace.append(torch.cuda.mem_get_info()[0])
    print(f"handle footprint {footprint / 2**20:.1f} MiB; free before {start / 2**20:.1f} MiB; after each cycle, relative: "
          + " ".join(f"{(t - start) / 2**20:+.1f}" for t in trace))
    assert footprint > 300 * 2**20, footprint  # (the method sees the handle's buffers at all)
    assert trace[-1] >= start - footprint // 2, (start, trace, footprint)


@pytest.mark.gpu
def test_graph_follows_replaced_buffers(system, monkeypatch):
    """NL_GRAPH=1: builds replayed from a captured graph stay right when the exclusion table is replaced by a larger one
    (new buffers: the graph must be captured again, buffers_epoch) and when it is cleared."""
    import torch

    from md_neighbor_list_amd import NeighListGPU

    monkeypatch.setenv("NL_GRAPH", "1")
    q, ref = system
    qd = torch.tensor(q).cuda()  # (a copy: q is read-only)
    nl = NeighListGPU(RC, *BOX, dtype=torch.float32)
    nl.Initialize(N)
    small = mixed_pairs(ref.key_pointer, ref.sorted_list, N, 3, k=300)
    large = mixed_pairs(ref.key_pointer, ref.sorted_list, N, 4, k=30000)
    nl.set_exclusions(small, N)
    for what in ("capture", "replay"):
        nl.MakeNeighList(qd, N, sync=False)
        nl.synchronize()
        _assert_list(nl, ref, small, what)
    old = tuple(int(t.data_ptr()) for t in nl.exclusions())
    nl.set_exclusions(large, N)
    assert tuple(int(t.data_ptr()) for t in nl.exclusions()) != old  # (the larger table did not fit the old buffers)
    for what in ("larger table", "larger table, replay"):
        nl.MakeNeighList(qd, N, sync=False)
        nl.synchronize()
        _assert_list(nl, ref, large, what)
    nl.clear_exclusions()
    for what in ("no table", "no table, replay"):
        nl.MakeNeighList(qd, N, sync=False)
        nl.synchronize()
        _assert_list(nl, ref, NO_PAIRS, what)


@pytest.mark.gpu
def test_failed_allocation_leaves_the_handle_usable(system):
    """A list capacity no device can hold is NL_ERR_NOMEM (the ordinary out-of-memory return of the allocation); a sane
    capacity after it, and a build, give the oracle's list."""
    import torch

    from md_neighbor_list_amd import NeighListGPU, _lib

    q, ref = system
    qd = torch.tensor(q).cuda()  # (a copy: q is read-only)
    nl = NeighListGPU(RC, *BOX, dtype=torch.float32)
    nl.Initialize(N)
    with pytest.raises(_lib.NLError) as err:
        nl.set_capacity(2**45)
    assert err.value.code == _lib.NL_ERR_NOMEM
    nl.set_capacity(ref.npairs + 1024)
    nl.MakeNeighList(qd, N)
    _assert_list(nl, ref, NO_PAIRS, "after the failed set_capacity")

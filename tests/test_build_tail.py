"""GPU tests of the build's fixed tail: the one-pass binning into row buckets (k_bin_bucket), the meta words the device
starts itself (no memset per build) and the launches of k_sweep_list_f32 / k_fill_list that a handle leaves out while
no cell needs them.  Every list is compared with the CPU oracle after the reference's canonical sort."""
import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.util import canonical_csr

pytestmark = pytest.mark.gpu

LIST_QUIET_BUILDS = 4  # nl_api.hip: builds after which a handle leaves the two launches out


def _po():
    from oracle import pyoracle as po

    return po


def _handle(rc, box, n_max, dtype=np.float32):
    import torch

    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box, dtype=torch.float32 if dtype == np.float32 else torch.float64)
    nl.Initialize(n_max)
    return nl


def _build(nl, q, sync=True):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(t, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    return t


def _check(nl, q, rc, box):
    ref = _po().build(q, rc, box)
    kp, sl = nl.key_pointer().cpu().numpy(), nl.sorted_list().cpu().numpy()
    assert nl.half_number_of_pairs() == ref.npairs
    assert int(kp[-1]) == ref.npairs
    assert np.array_equal(nl.half_number_of_partners().cpu().numpy(), ref.number_of_partners)
    assert np.array_equal(canonical_csr(kp, sl), ref.canonical().sorted_list)


def _slab_in_one_row(q, box, rc, extra, seed):
    """q plus `extra` particles spread along x inside the cell (y, z) = (3, 5): one row of x-cells far above the mean."""
    rng = np.random.default_rng(seed)
    m = [int(b / rc) for b in box]
    ms = [b / k for b, k in zip(box, m)]
    s = np.zeros((extra, 4), dtype=q.dtype)
    s[:, 0] = rng.uniform(0.0, box[0] * (1 - 1e-6), extra)
    s[:, 1] = (3 + rng.uniform(0.05, 0.95, extra)) * ms[1]
    s[:, 2] = (5 + rng.uniform(0.05, 0.95, extra)) * ms[2]
    return np.concatenate([q, s])


def _cluster(q, box, rc, per_cell, seed):
    """q plus a block of 3 x 3 x 3 cells at `per_cell` extra particles each: stencil streams beyond the LDS buffer, rows
    within their buckets."""
    rng = np.random.default_rng(seed)
    m = [int(b / rc) for b in box]
    ms = [b / k for b, k in zip(box, m)]
    k = 27 * per_cell
    s = np.zeros((k, 4), dtype=q.dtype)
    for d in range(3):
        s[:, d] = (4 + rng.uniform(0.01, 2.99, k)) * ms[d]
    return np.concatenate([q, s])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_past_its_bucket_runs_again_once(dtype):
    """A dense slab in one y/z row overflows its bucket: the build runs again with the two-pass binning and is exact;
    the handle's next build has buckets twice as large and needs no second run."""
    rc, box = 3.3, (40.0, 40.0, 40.0)
    q0, _ = inputs.uniform_box(30000, dtype=dtype, seed=71, box=box)
    q = _slab_in_one_row(q0, box, rc, 600, seed=72)  # the row: ~808 particles, mean 208 (bucket 516)
    nl = _handle(rc, box, len(q), dtype)
    _build(nl, q0)
    _check(nl, q0, rc, box)
    first = nl.build_stats()
    assert first["row_overflow_reruns"] == 0 and first["cap_row"] > 0
    _build(nl, q)
    _check(nl, q, rc, box)
    st = nl.build_stats()
    assert st["row_overflow_reruns"] == 1
    _build(nl, q)
    _check(nl, q, rc, box)
    st = nl.build_stats()
    assert st["row_overflow_reruns"] == 1 and st["cap_row"] >= 2 * first["cap_row"] - 2


@pytest.mark.parametrize("buckets", ["0", "1"])
def test_list_launches_come_back_when_a_stream_exceeds_the_buffer(buckets, monkeypatch):
    """Sparse builds hand no cell to k_sweep_list_f32 / k_fill_list, and the handle leaves their launches out; a build
    with streams beyond the LDS buffer is still exact (run again with the launches), the next one launches them, and
    an asynchronous build of such a box is exact after synchronize."""
    monkeypatch.setenv("NL_BIN_BUCKETS", buckets)
    rc, box = 3.3, (60.0, 60.0, 60.0)  # 18^3 cells, ~9 particles a cell
    q0, _ = inputs.uniform_box(52000, dtype=np.float32, seed=81, box=box)
    q = _cluster(q0, box, rc, 60, seed=82)  # the block's cells: ~69 particles, streams up to ~1860
    nl = _handle(rc, box, len(q))
    for _ in range(LIST_QUIET_BUILDS + 2):
        _build(nl, q0)
    _check(nl, q0, rc, box)
    st = nl.build_stats()
    assert not st["list_launched"] and st["list_reruns"] == 0
    assert (st["cap_row"] > 0) == (buckets == "1")
    _build(nl, q)
    _check(nl, q, rc, box)
    st = nl.build_stats()
    assert st["list_reruns"] == 1 and st["list_launched"]
    _build(nl, q)
    _check(nl, q, rc, box)
    st = nl.build_stats()
    assert st["list_reruns"] == 1 and st["list_launched"]
    for _ in range(LIST_QUIET_BUILDS + 1):
        _build(nl, q0)
    assert not nl.build_stats()["list_launched"]
    _build(nl, q, sync=False)
    _check(nl, q, rc, box)
    assert nl.build_stats()["list_reruns"] == 2


def test_one_handle_many_sizes_and_positions():
    """Builds of different N and positions on one handle, with failures in between and no host reset: the device
    starts the status word, the tickets and the totals of every build itself."""
    import torch

    from md_neighbor_list_amd import NLError
    from md_neighbor_list_amd import _lib

    rc, box = 3.3, (36.0, 33.0, 30.0)
    nl = _handle(rc, box, 40000)
    for k, n in enumerate([40000, 7000, 25000, 1, 31000, 40000, 12000]):
        q, _ = inputs.uniform_box(n, dtype=np.float32, seed=90 + k, box=box)
        _build(nl, q, sync=k % 2 == 0)
        _check(nl, q, rc, box)
        if k == 2:
            bad = q.copy()
            bad[17, 1] = 99.0
            with pytest.raises(NLError) as e:
                nl.MakeNeighList(torch.from_numpy(bad).cuda(), n, sync=True)
            assert e.value.code == _lib.NL_ERR_OUT_OF_BOX
    # an undersized list: the asynchronous build fails, the synchronous one grows it
    nl.set_capacity(1000)
    t = torch.from_numpy(q).cuda()
    nl.MakeNeighList(t, len(q), sync=False)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == _lib.NL_ERR_CAPACITY
    nl.MakeNeighList(t, len(q), sync=True)
    _check(nl, q, rc, box)
    assert nl.build_stats()["row_overflow_reruns"] == 0


def test_back_to_back_asynchronous_builds():
    """Two asynchronous builds in a row, then one synchronize: the list is the second box's."""
    import torch

    rc, box = 3.3, (40.0, 40.0, 40.0)
    qa, _ = inputs.uniform_box(60000, dtype=np.float32, seed=101, box=box)
    qb, _ = inputs.uniform_box(55000, dtype=np.float32, seed=102, box=box)
    nl = _handle(rc, box, 60000)
    ta, tb = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
    for _ in range(3):
        nl.MakeNeighList(ta, len(qa), sync=False)
        nl.MakeNeighList(tb, len(qb), sync=False)
        nl.synchronize()
        _check(nl, qb, rc, box)


@pytest.mark.parametrize("dtype,rows", [(np.float32, "4"), (np.float64, "-1")])
def test_fine_rows_and_fp64_through_the_buckets(dtype, rows, monkeypatch):
    """The fine-row layout (k_bin_cells<FINE> on the buckets) and an fp64 box through the one-pass binning."""
    monkeypatch.setenv("NL_ROWS", rows)
    rc, box = 3.3, (36.84, 36.84, 36.84)
    q, _ = inputs.uniform_box(50000, dtype=dtype, seed=111, box=box)
    nl = _handle(rc, box, len(q), dtype)
    for _ in range(2):
        _build(nl, q)
        _check(nl, q, rc, box)
    assert nl.build_stats()["cap_row"] > 0
    if rows == "4":
        assert nl.build_info()["fine_rows"] > 0

"""GPU tests of the Verlet-skin update (nl_update_list): the rebuild decision taken on the device, the gated build, the
snapshot it keeps, graph replays, and forces enqueued without a host wait.  Every list is compared with the CPU oracle
after the reference's canonical sort; every rebuild decision with a numpy replay of the rule of include/nl_hip.h."""
import os
import sys

import numpy as np
import pytest

from md_neighbor_list_amd import inputs
from tests.util import ROOT, canonical_csr

pytestmark = pytest.mark.gpu


def _po():
    from oracle import pyoracle as po

    return po


def _torch():
    import torch

    return torch


def _handle(rc, box, n_max, dtype, skin, full=False, pbc=False):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(rc, *box, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=pbc)
    nl.Initialize(n_max)
    nl.set_skin(skin)
    return nl


def _full_from_half(h):
    n = len(h.key_pointer) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(h.key_pointer))
    cols = h.sorted_list.astype(np.int64)
    a, b = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    key = (a << 32) | b
    key.sort()
    return (key & 0xFFFFFFFF).astype(np.int32)


def _check(nl, q, rc, box):
    """The handle's list equals the oracle's list of positions q."""
    po = _po()
    if nl.full_list:
        kp, lst, _ = (t.cpu().numpy() for t in nl.full_csr())
        want = po.build_pbc_full(q, rc, box).sorted_list if nl.minimum_image else _full_from_half(po.build(q, rc, box))
        assert np.array_equal(canonical_csr(kp, lst), want)
        return
    ref = po.build_pbc(q, rc, box) if nl.minimum_image else po.build(q, rc, box).canonical()
    kp, sl = nl.key_pointer().cpu().numpy(), nl.sorted_list().cpu().numpy()
    assert int(kp[-1]) == ref.npairs
    assert np.array_equal(nl.half_number_of_partners().cpu().numpy(), ref.number_of_partners)
    assert np.array_equal(canonical_csr(kp, sl), ref.sorted_list)


def _state(nl):
    """Every array a skipped update must leave byte-identical."""
    cs, sr = nl.sorted_state()
    if nl.full_list:
        kp, lst, cnt = (t.cpu().numpy().copy() for t in nl.full_csr())
    else:
        kp, lst, cnt = (t.cpu().numpy().copy() for t in (nl.key_pointer(), nl.sorted_list(), nl.half_number_of_partners()))
    return [kp, lst, cnt, cs.cpu().numpy().copy(), sr.cpu().numpy().copy()]


def _r2(q, snap, box, pbc):
    """Rule (c): d in the position type, then double; minimum image in double; (dx^2 + dy^2) + dz^2 without FMA."""
    d = (q[:, :3] - snap[:, :3]).astype(np.float64)  # (numpy subtracts in the arrays' type, rounded to nearest)
    if pbc:
        L = np.array(box, dtype=np.float64)
        d = d - L * np.rint(d / L)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _replay(seq, skin, box, pbc=False):
    """Steps of seq[1:] at which rule (c) rebuilds, seq[0] being the first (forced) build; and the last snapshot."""
    thr = (0.5 * skin) ** 2
    snap, steps = seq[0], []
    for k in range(1, len(seq)):
        r2 = _r2(seq[k], snap, box, pbc)
        if np.isnan(r2).any() or r2.max() > thr:
            steps.append(k)
            snap = seq[k]
    return steps, snap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("pbc", [False, True])
def test_first_update_builds_the_oracle_list(dtype, full, pbc):
    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=dtype, seed=21, box=(28.0, 28.0, 28.0))
    nl = _handle(3.3, box, len(q), dtype, 0.4, full, pbc)
    nl.update(torch.from_numpy(q).cuda())
    nl.synchronize()
    assert nl.update_stats() == (1, 1)
    _check(nl, q, 3.3, box)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moves_below_half_the_skin_change_nothing(dtype):
    torch = _torch()
    rng = np.random.default_rng(3)
    rc, skin = 3.3, 0.6
    q0, box = inputs.uniform_box(20000, dtype=dtype, seed=22, box=(28.0, 28.0, 28.0))
    nl = _handle(rc, box, len(q0), dtype, skin)
    qd = torch.from_numpy(q0).cuda()
    nl.update(qd, sync=True)
    before = _state(nl)
    for k in range(3):  # random moves, each particle less than skin/2 from the snapshot
        q = q0.copy()
        step = rng.normal(size=(len(q), 3))
        step *= (0.45 * 0.5 * skin * rng.random((len(q), 1))) / np.linalg.norm(step, axis=1, keepdims=True)
        q[:, :3] = np.clip(q0[:, :3] + step.astype(dtype), 0, np.nextafter(box[0], 0)).astype(dtype)
        assert _r2(q, q0, box, False).max() <= (0.5 * skin) ** 2
        qd.copy_(torch.from_numpy(q))
        nl.update(qd)
        nl.synchronize()
        assert nl.update_stats() == (2 + k, 1)
        after = _state(nl)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    # one particle past skin/2: a rebuild, and the list of the NEW positions
    q[7, 0] = q0[7, 0] + dtype(0.51 * skin) if q0[7, 0] < 20 else q0[7, 0] - dtype(0.51 * skin)
    qd.copy_(torch.from_numpy(q))
    nl.update(qd)
    nl.synchronize()
    assert nl.update_stats() == (5, 2)
    _check(nl, q, rc, box)


def test_drift_accumulates_against_the_snapshot():
    torch = _torch()
    skin = 0.5
    q, box = inputs.uniform_box(4096, dtype=np.float32, seed=23, box=(16.0, 16.0, 16.0))
    q[0, :3] = (2.0, 8.0, 8.0)
    nl = _handle(3.2, box, len(q), np.float32, skin)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd)
    seq, built = [q.copy()], []
    for k in range(1, 11):
        q[0, 0] += np.float32(0.3 * 0.5 * skin)
        seq.append(q.copy())
        qd.copy_(torch.from_numpy(q))
        b0 = nl.update_stats()[1]
        nl.update(qd)
        if nl.update_stats()[1] > b0:
            built.append(k)
    # against the previous step (0.3 skin/2) it would never build; against the first build, at every step from the 4th
    assert built == _replay(seq, skin, box)[0] == [4, 8]
    nl.synchronize()
    _check(nl, q if built[-1] == 10 else seq[built[-1]], 3.2, box)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_threshold(dtype):
    from md_neighbor_list_amd._lib import NL_ERR_OUT_OF_BOX, NLError

    torch = _torch()
    q, box = inputs.uniform_box(4096, dtype=dtype, seed=24, box=(16.0, 16.0, 16.0))
    q[0, :3] = (1.0, 5.0, 5.0)
    nl = _handle(3.2, box, len(q), dtype, 0.5)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    q[0, 0] = dtype(1.25)  # r2 = 0.0625 = (skin/2)^2 exactly: not past it
    qd.copy_(torch.from_numpy(q))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 1)
    q[0, 0] = np.nextafter(dtype(1.25), dtype(2))
    qd.copy_(torch.from_numpy(q))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (3, 2)
    _check(nl, q, 3.2, box)
    q[9, 1] = np.nan
    qd.copy_(torch.from_numpy(q))
    nl.update(qd)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_OUT_OF_BOX
    assert nl.update_stats() == (4, 3)


@pytest.mark.parametrize("pbc", [False, True])
def test_periodic_crossing(pbc):
    torch = _torch()
    L = 16.0
    q, box = inputs.uniform_box(4096, dtype=np.float32, seed=25, box=(L, L, L))
    q[3, :3] = (L - 0.01, 6.0, 6.0)
    q0 = q.copy()
    nl = _handle(3.2, box, len(q), np.float32, 0.5, pbc=pbc)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    q[3, 0] = np.float32(0.01)  # the caller wrapped it into the box: 0.02 by the minimum image, L - 0.02 in an open box
    qd.copy_(torch.from_numpy(q))
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 1 if pbc else 2)
    _check(nl, q0 if pbc else q, 3.2, box)


def _walk(n, steps, dtype, seed, box, sigma):
    q, _ = inputs.uniform_box(n, dtype=dtype, seed=seed, box=box)
    rng = np.random.default_rng(seed)
    seq = [q]
    pos = q[:, :3].astype(np.float64)
    for _ in range(steps):
        pos = np.clip(pos + rng.normal(0.0, sigma, size=pos.shape), 0.0, box[0] * (1 - 1e-6))
        nxt = q.copy()
        nxt[:, :3] = pos.astype(dtype)
        seq.append(nxt)
    return seq


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_async_updates_on_one_stream(graph, dtype):
    torch = _torch()
    box, rc, skin = (20.0, 20.0, 20.0), 3.3, 0.6
    seq = _walk(6000, 200, dtype, 26, box, 0.01)
    dev = torch.from_numpy(np.stack(seq)).cuda()  # every position set up front
    nl = _handle(rc, box, len(seq[0]), dtype, skin)
    nl.set_graph(graph)
    qd = dev[0].clone()
    nl.update(qd)
    for k in range(1, len(seq)):
        qd.copy_(dev[k], non_blocking=True)
        nl.update(qd)
    nl.synchronize()
    steps, snap = _replay(seq, skin, box)
    assert 3 <= len(steps) < 150  # (the walk rebuilds now and then, not always)
    assert nl.update_stats() == (len(seq), 1 + len(steps))
    _check(nl, snap, rc, box)


def test_host_known_reasons_force_a_build():
    torch = _torch()
    rc = 3.3
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=27, box=(28.0, 28.0, 28.0))
    nl = _handle(rc, box, len(q), np.float32, 0.4)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd, sync=True)
    nl.update(qd, sync=True)
    assert nl.update_stats() == (2, 1)
    two_pairs = np.array([[0, 1], [5, 2]], dtype=np.int32)
    two_types = (np.arange(len(q)) % 2).astype(np.int32)
    # every cause rule (a) of include/nl_hip.h names, each followed by an update that builds and one that does not
    setters = [lambda: nl.set_capacity(40_000_000), lambda: nl.set_offset_width(0), lambda: nl.set_periodic(False),
               lambda: nl.set_full_list(False), lambda: nl.set_skin(0.4), lambda: nl.Initialize(len(q)),
               lambda: nl.MakeNeighList(qd, len(q)),
               lambda: nl.set_periodic(axes="xy"), lambda: nl.set_periodic(False),
               lambda: nl.set_pair_images(True), lambda: nl.set_pair_images(False),
               lambda: nl.set_exclusions(two_pairs, len(q)), lambda: nl.clear_exclusions(),
               lambda: nl.set_type_cutoffs(two_types, np.full((2, 2), rc)), lambda: nl.clear_type_cutoffs(),
               lambda: nl.set_box(28.3, 28.0, 28.0), lambda: nl.set_box(*box),  # (8 cells a side either way)
               lambda: nl.profile_last_build(reps=1), lambda: nl.profile_stages(qd, reps=1)]
    for k, setter in enumerate(setters):
        setter()
        nl.update(qd, sync=True)
        assert nl.update_stats() == (3 + 2 * k, 2 + k), k
        nl.update(qd, sync=True)  # and the one after it does not
        assert nl.update_stats() == (4 + 2 * k, 2 + k), k
    _check(nl, q, rc, box)
    # nl_resort: the particles permuted into the build's cell order; the update builds the list of the permuted input
    order = nl.cell_order().cpu().numpy().copy()
    nl.resort(qd)
    b = nl.update_stats()[1]
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == b + 1
    assert np.array_equal(qd.cpu().numpy(), q[order])
    _check(nl, q[order], rc, box)


def test_capacity_overflow():
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    rc = 3.3
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = _handle(rc, box, len(q), np.float32, 0.4)
    nl.set_capacity(1000)
    qd = torch.from_numpy(q).cuda()
    nl.update(qd)
    f = nl.lj_forces(qd, wait=False)  # stream-ordered behind the failed build: NaN
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert torch.isnan(f).all()
    nl.update(qd)  # the host has seen the failure: builds (and fails) again
    with pytest.raises(NLError):
        nl.synchronize()
    assert nl.update_stats() == (2, 2)
    nl.update(qd, sync=True)  # grows the list
    assert nl.update_stats() == (3, 3)
    _check(nl, q, rc, box)
    f = nl.lj_forces(qd, wait=False)
    assert torch.isfinite(f).all()


def _md_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import md_loop
    finally:
        sys.path.pop(0)
    return md_loop


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_md_equivalence(dtype):
    torch = _torch()
    md = _md_loop()
    cells, a = 6, 1.56
    box = 4.0 * cells
    q, v = md.fcc_droplet(cells, a, box, dtype)
    sim = md.Simulation(q, v, box, trigger="host")
    rc, skin = sim.rc, sim.skin
    seq, forces, host_builds = [sim.q.cpu().numpy().copy()], [sim.f.cpu().numpy().copy()], []
    for k in range(1, 301):
        b = sim.builds
        sim.step()
        seq.append(sim.q.cpu().numpy().copy())
        forces.append(sim.f.cpu().numpy().copy())
        if sim.builds > b:
            host_builds.append(k)
    assert sim.sorts == 0  # (no re-sort inside 300 steps: the positions are one particle order)
    steps, _ = _replay(seq, skin, (box,) * 3)
    assert len(steps) >= 2
    # the host trigger sums in the position type: equal up to a last-ulp tie at the threshold
    assert len(set(steps) ^ set(host_builds)) <= 2
    rtol = 1e-5 if dtype == np.float32 else 1e-12

    def close(f, k):
        want = forces[k]
        np.testing.assert_allclose(f, want, rtol=rtol, atol=rtol * np.abs(want).max(), err_msg=f"step {k}")

    tdt = torch.float32 if dtype == np.float32 else torch.float64
    dev = torch.from_numpy(np.stack(seq)).cuda()
    # update + forces without a host wait, step by step
    nl = _handle(rc + skin, (box,) * 3, len(q), dtype, skin, full=True)
    qd = dev[0].clone()
    nl.update(qd)
    close(nl.lj_forces(qd, rc_force=rc, wait=False).cpu().numpy(), 0)
    built = []
    for k in range(1, len(seq)):
        b = nl.update_stats()[1]
        qd.copy_(dev[k])
        nl.update(qd)
        f = nl.lj_forces(qd, rc_force=rc, wait=False)
        if nl.update_stats()[1] > b:
            built.append(k)
        close(f.cpu().numpy(), k)
    assert built == steps
    # one step captured in a graph, replayed 300 times
    nl = _handle(rc + skin, (box,) * 3, len(q), dtype, skin, full=True)
    src = dev[0].clone()
    qd = dev[0].clone()
    fd = torch.empty((len(q), 4), dtype=tdt, device="cuda")
    nl.update(qd, sync=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        nl.lj_forces(qd, rc_force=rc, wait=False, out=fd)
    built = []
    for k in range(1, len(seq)):
        b = nl.update_stats()[1]
        src.copy_(dev[k])
        g.replay()
        torch.cuda.synchronize()
        if nl.update_stats()[1] > b:
            built.append(k)
        close(fd.cpu().numpy(), k)
    assert built == steps

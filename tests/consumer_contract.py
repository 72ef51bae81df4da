"""What every table-driven consumer of the list (pair table, embedded-atom, Stillinger-Weber) promises a caller beyond its
numbers, stated once: enqueue behind nl_update_list, graph capture, a failed list gives NaN, the list's reach, which lists are
refused, and the state and argument rules of the four entry points.

A family describes itself with a Consumer; the functions below take it and the parameters of the test.  Each test keeps its
name, decorators and parametrisation in its family's file and calls one function here.  The inputs are the table family's of
tests.consumer_util: the 2744-particle lattice, and the 20000-particle box of seed 28 for the failed list.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from tests.consumer_util import N, _handle, _tdt, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.util import LJ_BOXES

# forces, virial, scratch, clear, info: names of NeighListGPU methods -- the per-row output, the totals, the call that
#   allocates scratch on its first use, the clearing call and the getter;
# entry: the C entry points (forces, forces_enqueue, virial, virial_enqueue);
# set(nl, kind, rc, **kw): the type table of `kind` at the list's cut-off rc and the family's tables onto an initialised handle;
# kinds: the potentials, the first of one type; ref(box, drift, kind), moved_ref(box, kind): their references;
# extra(nl): the outputs beyond forces and totals, a tuple of (n,) device tensors (the EAM rho and fp; else empty);
# check(f, w, extra, ref, dtype, rows=None): all outputs within the family's bounds;
# half_lists, local_slabs: whether half lists and local-index slab lists are accepted.
Consumer = collections.namedtuple("Consumer", "forces virial scratch clear info entry set kinds ref moved_ref extra check "
                                              "half_lists local_slabs")


def entry_calls(d, lib, fd, out):
    """[(C function, its output)] of the four entry points: fd for the rows, out for the totals."""
    return [(getattr(lib, name), o) for name, o in zip(d.entry, (fd, fd, out, out))]


def built(d, q, box, dtype, full, rc, kind, off=0, stride=4, **kw):
    """(handle, device positions) after one build, the tables set."""
    torch = _torch()
    nl = _handle(box, dtype, full, rc, off)
    nl.Initialize(len(q))
    d.set(nl, kind, rc, **kw)
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


def run(d, nl, qd, ref, dtype, wait=True, rows=None):
    """Forces, the extra outputs and the totals of one list, their shapes and types, and the family's check; returns what the
    check returns (the outputs on the host)."""
    f = getattr(nl, d.forces)(qd, wait=wait)
    x = d.extra(nl)
    w = getattr(nl, d.virial)(qd, wait=wait)
    assert f.shape == (len(qd), 4) and f.dtype == _tdt(dtype) and w.shape == (8,) and w.dtype == _torch().float64
    assert all(v.shape == (len(qd),) and v.dtype == _tdt(dtype) for v in x)
    return d.check(f, w, x, ref, dtype, rows)


# ------------------------------------------------------------------------------------------------------ the contract
def reuse_within_the_skin(d, box, kind, full, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variants; no extra build."""
    torch = _torch()
    q1 = _moved(box)[0]
    nl = _handle(box, dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    d.set(nl, kind, 2.9)
    qd = torch.from_numpy(_input(box, False).astype(dtype)).cuda()
    nl.update(qd, sync=True)
    builds = nl.update_stats()[1]
    getattr(nl, d.scratch)(qd)  # (the scratch)
    qd.copy_(torch.from_numpy(q1.astype(dtype)))
    nl.update(qd)
    f = getattr(nl, d.forces)(qd, wait=False)
    x = d.extra(nl)
    w = getattr(nl, d.virial)(qd, wait=False)
    torch.cuda.synchronize()
    assert nl.update_stats()[1] == builds
    d.check(f, w, x, d.moved_ref(box, kind), dtype)


def captured(d, full, before, after):
    """One graph holds the copy of the positions, the update, the forces and the totals; replayed at two position sets.
    before(nl, qd, fd, wd) runs between the enqueued update and the capture: whatever makes the scratch exist, and what the
    family refuses until it does.  after(nl, replay) runs behind the two replays; replay() runs the graph once more on cleared
    outputs and returns (fd, wd)."""
    torch = _torch()
    dtype = np.float32
    kind = d.kinds[0]
    sets = [(_input("xyz", False), d.ref("xyz", False, kind)), (_moved("xyz")[0], d.moved_ref("xyz", kind))]
    nl = _handle("xyz", dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    d.set(nl, kind, 2.9)
    src = torch.from_numpy(sets[0][0].astype(dtype)).cuda()
    qd = src.clone()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    nl.update(qd, sync=True)
    nl.update(qd)
    before(nl, qd, fd, wd)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        getattr(nl, d.forces)(qd, wait=False, out=fd)
        getattr(nl, d.virial)(qd, wait=False, out=wd)

    def replay():
        fd.fill_(-1.0), wd.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        return fd, wd

    for q, ref in sets:
        src.copy_(torch.from_numpy(q.astype(dtype)))
        replay()
        d.check(fd, wd, d.extra(nl), ref, dtype)
    after(nl, replay)


def failed_list(d, set_tables, prepare):
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN in every output, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat all are finite.  set_tables(nl): tables that start near 0 (a uniform random box
    has close pairs); prepare(nl, qd): the family's calls before the capacity shrinks (its scratch)."""
    from md_neighbor_list_amd import NeighListGPU, inputs
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=not d.half_lists)
    nl.set_skin(0.4)
    nl.Initialize(len(q))
    set_tables(nl)
    qd = torch.from_numpy(q).cuda()
    prepare(nl, qd)
    nl.set_capacity(1000)
    nl.update(qd)
    f, w = getattr(nl, d.forces)(qd, wait=False), getattr(nl, d.virial)(qd, wait=False)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert torch.isnan(f).all() and f.shape == (len(q), 4) and torch.isnan(w).all() and w.shape == (8,)
    assert all(torch.isnan(v).all() for v in d.extra(nl))
    nl.update(qd, sync=True)  # grows the list
    f, w = getattr(nl, d.forces)(qd, wait=False), getattr(nl, d.virial)(qd, wait=False)
    assert torch.isfinite(f).all() and torch.isfinite(w).all() and w[7] > 0


def both_offset_widths(d, full, off):
    kind = d.kinds[-1]
    nl, qd = built(d, _input("hex", True), "hex", np.float32, full, 2.5, kind, off)
    assert nl.build_info()["offset_bits"] == off
    run(d, nl, qd, d.ref("hex", True, kind), np.float32)


def slab_lists_are_refused(d, full):
    """A slab build, with and without nl_set_local_ids: NL_ERR_STATE from all four calls."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError
    from tests.test_slab_paths import slab_parts

    assert not d.local_slabs
    torch = _torch()
    box, dtype, rc = "xyz", np.float32, 3.4
    box6, mask = LJ_BOXES[box]
    q = _input(box, False)
    part = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 2), (2, 4)), mask)[0]
    for local in (True, False):
        nl = _handle(box, dtype, full, rc)
        nl.set_local_ids(local)
        nl.Initialize(N)
        d.set(nl, d.kinds[0], rc)
        qd = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
        nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"])
        if local:
            assert torch.isfinite(nl.table_forces(qd)).all()  # (the pair table's calls take this list)
        for call in (getattr(nl, d.forces), getattr(nl, d.virial)):
            for wait in (True, False):
                with pytest.raises(NLError) as e:
                    call(qd, wait=wait)
                assert e.value.code == NL_ERR_STATE


def distributed_lists_are_refused(d, full):
    """A distributed build of a world of one (nl_make_list_distributed: the whole box, the global ids in w): its list holds
    caller ids, and all four calls are NL_ERR_STATE, wait and enqueue."""
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd._lib import NL_ERR_STATE

    torch = _torch()
    box, dtype, rc = "xyz", np.float32, 3.4
    nl = _handle(box, dtype, full, rc)
    nl.Initialize(N)
    d.set(nl, d.kinds[0], rc)
    lib = nl._lib
    q = _input(box, False).astype(np.float32)
    q[:, 3] = np.arange(N, dtype=np.int32).view(np.float32)  # NL_GID_IN_W
    qd = torch.from_numpy(q).cuda()
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    cb = _lib.SENDRECV_FN(lambda *a: 1)  # (never called: a world of one exchanges nothing)
    comm = C.c_void_p()
    assert lib.nl_comm_create_callbacks(C.byref(comm), 0, 1, cb, None, torch.cuda.current_device()) == 0
    try:
        assert lib.nl_make_list_distributed(nl._h, comm, qd.data_ptr(), N, N, None, 1) == 0
        npairs = C.c_int64()
        assert lib.nl_number_of_pairs(nl._h, C.byref(npairs)) == 0 and npairs.value > 50 * N  # (the build succeeded: about 55 pairs a particle)
        for fn, o in entry_calls(d, lib, fd, out):
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    finally:
        lib.nl_comm_destroy(comm)


# --------------------------------------------------------------------- the blocks of a family's test_state_and_arguments
def call_arguments(calls, nl, qd):
    """The four entry points against a null out, null q, a null handle and the strides 0, 2 and 5."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG

    for fn, o in calls:
        assert fn(nl._h, qd.data_ptr(), 4, None, None) == NL_ERR_ARG
        assert fn(nl._h, None, 4, o.data_ptr(), None) == NL_ERR_ARG
        assert fn(None, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_ARG
        for stride in (0, 2, 5):
            assert fn(nl._h, qd.data_ptr(), stride, o.data_ptr(), None) == NL_ERR_ARG


def setter_keeps_the_list(nl, qd, set_again):
    """The setter does not touch the list: an update after it builds nothing."""
    nl.update(qd, sync=True)
    builds = nl.update_stats()[1]
    set_again()
    nl.update(qd, sync=True)
    assert nl.update_stats()[1] == builds


def reach(d, nl, qd, set_r_max):
    """rc = 2.9, skin = 0.3 -- r_max = 2.6 is within rc and within rc - skin, 2.7 and 2.9 only within rc, 3.0 within neither.
    set_r_max(r_max): the family's tables ending at r_max.  Only the status is looked at."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NLError

    for r_max, sync_ok, enq_ok in ((2.6, True, True), (2.7, True, False), (2.9, True, False), (3.0, False, False)):
        set_r_max(r_max)
        for wait, ok in ((True, sync_ok), (False, enq_ok)):
            for call in (getattr(nl, d.forces), getattr(nl, d.virial)):
                if ok:
                    call(qd, wait=wait)
                else:
                    with pytest.raises(NLError) as e:
                        call(qd, wait=wait)
                    assert e.value.code == NL_ERR_ARG, (r_max, wait)


def clearing(d, nl, qd, set_again, set_no_knots):
    """Clearing, both ways: the wrapper's call, and the setter with 0 knots (set_no_knots() returns its status); then the
    calls are NL_ERR_STATE."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    getattr(nl, d.clear)()
    assert getattr(nl, d.info)() is None
    set_again()
    assert set_no_knots() == 0 and getattr(nl, d.info)() is None
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            getattr(nl, d.forces)(qd, wait=wait)
        assert e.value.code == NL_ERR_STATE


def several_types(d, nl, qd, types, set_one, set_three):
    """Tables of three types need a type table of three types; tables of one type work with any.  The last type table has
    rc_ab = 2.55 for one pair, short of r_max + skin = 2.5 + 0.3: the blocking call takes it, the enqueue does not."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    torch = _torch()
    forces, virial = getattr(nl, d.forces), getattr(nl, d.virial)
    set_three()
    for call in (forces, virial):
        with pytest.raises(NLError) as e:
            call(qd)
        assert e.value.code == NL_ERR_STATE
    nl.set_type_cutoffs(types % 2, [[2.9, 2.9], [2.9, 2.9]])
    nl.MakeNeighList(qd, N)
    with pytest.raises(NLError) as e:
        forces(qd)
    assert e.value.code == NL_ERR_ARG  # ntypes 3 against the type table's 2
    set_one()
    assert torch.isfinite(forces(qd)).all()  # one type works with a type table set
    nl.set_type_cutoffs(types, [[2.9, 2.9, 0.0], [2.9, 2.55, 2.9], [0.0, 2.9, 2.9]])  # rc_ab: one pair short of r_max + skin
    nl.MakeNeighList(qd, N)
    set_three()
    assert torch.isfinite(virial(qd)).all()  # 2.5 <= 2.55; the pair with rc_ab = 0 has no entries
    with pytest.raises(NLError) as e:
        virial(qd, wait=False)  # 2.5 > 2.55 - 0.3
    assert e.value.code == NL_ERR_ARG


def no_particles(d, lib, full, set_tables, qd, fd, out):
    """n == 0: both blocking calls succeed and the totals are 8 zeros."""
    torch = _torch()
    empty = _handle("open", np.float32, full, 2.9)
    empty.Initialize(16)
    set_tables(empty)
    empty.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    out.fill_(7.0)  # (an empty tensor has no address to pass: the positions are not read)
    assert getattr(lib, d.entry[2])(empty._h, qd.data_ptr(), 4, out.data_ptr(), None) == 0
    assert getattr(lib, d.entry[0])(empty._h, qd.data_ptr(), 4, fd.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.zeros(8))

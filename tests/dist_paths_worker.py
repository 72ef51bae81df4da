"""Worker of tests/test_distributed_paths.py: nl_make_list_distributed on every rank of a gloo world (host transport,
the ranks share the device), each rank checked on its own, row by row, against the oracle's list of the undivided box.

Ranks must never desynchronise (the host transport blocks): a mismatch is recorded as a message and the rank goes on; a
library error a configuration does not expect is recorded too, and a flag gathered after EVERY build makes all ranks
leave the remaining configurations at the same collective call.  At the end of each configuration the ranks gather
their messages; after the last one rank 0 reports ("ok", ...) or ("fail", messages).

The tables of configurations (TESTS) are shared with the CPU test, which checks the expectations themselves.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from md_neighbor_list_amd import slab  # noqa: E402
from tests.test_periodic_axes import positions  # noqa: E402
from tests.test_slab_paths import (BOXES, RC, check_rows, expected_plan, global_list, list_of, make_handle, make_input,  # noqa: E402
                                   mesh, mix_sum, read_slab, slab_parts)

MASK64 = 2**64 - 1
VACATED_LAYER = 4  # of box A, world 5 (2 + 2 + 1 + 1 + 1): the one layer of rank 2
CROWD_EXTRAS = (1300, 1900, 2500, 3100, 3700)


class Abort(Exception):
    """Some rank met a library error its configuration does not expect: every rank leaves at the same build."""


# ------------------------------------------------------------------------------------------------------ inputs


@functools.lru_cache(maxsize=None)
def get_input(key):
    """Positions [n, 4] (read-only) of a key: the keys of make_input, and
    (box, n, dtype, "edges", mask): tests.test_periodic_axes.positions (particles just outside every face the mask wraps,
        open-axis coordinates in [0, L + rc/2): what the padded reference of a mixed mask needs);
    (box, per_cell, dtype, "vacated", 0): uniform without the particles of layer VACATED_LAYER;
    (box, per_cell, dtype, "moved", base): the input (box, per_cell, dtype, *base) with every particle moved by up to 0.45
        cells and wrapped into the box (as worker_cabi of tests/slab_worker.py moves them)."""
    box_name, per_cell, dtype, kind, extra = key
    box = BOXES[box_name]
    dt = np.dtype(dtype).type
    if kind == "edges":
        q = positions(per_cell, box, RC, extra, dt, 40 + extra + (500 if dt == np.float64 else 0))
    elif kind == "vacated":
        q = make_input(box_name, per_cell, dtype, "uniform", 0)
        q = np.ascontiguousarray(q[layers_of(q, box, 0) != VACATED_LAYER])
    elif kind == "moved":
        q = np.array(get_input((box_name, per_cell, dtype) + tuple(extra)))
        rng = np.random.default_rng(5)
        q[:, :3] += rng.uniform(-1.5, 1.5, size=(len(q), 3)).astype(dt)
        q[:, :3] = np.mod(q[:, :3], np.array(box, dtype=dt))
        q[:, :3] = np.minimum(q[:, :3], np.nextafter(np.array(box, dtype=dt), dt(0)))
    else:
        return make_input(*key)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def get_list(key, mask, full):
    """(counts, key_pointer, list) of the undivided box for a key of get_input: the oracle alone."""
    if key[3] in ("edges", "vacated", "moved"):
        return list_of(get_input(key), BOXES[key[0]], mask, full)
    return global_list(key, mask, full)


@functools.lru_cache(maxsize=None)
def list_sum(key, mask, full):
    cnt, _, lst = get_list(key, mask, full)
    return mix_sum(np.arange(len(cnt)), cnt, lst)


def layers_of(q, box, mask):
    import torch

    return slab.z_layer(torch.from_numpy(np.array(q)), box, RC, periodic_z=bool(mask & 4)).numpy()


def parts_of(key, mask, world):
    box = BOXES[key[0]]
    return slab_parts(get_input(key), box, RC, slab.split_layers(mesh(box)[2], world), mask)


def halo_capacity(count):
    """nl_dist.inc: the capacity negotiated for a layer of `count` particles."""
    return count + count // 4 + 1024


@functools.lru_cache(maxsize=None)
def crowd_extra(dtype, world=2):
    """The smallest `extra` of the crowd input on box C with which a layer at the cut outgrows the capacity its message
    was negotiated for with the uniform part alone."""
    uni = parts_of(("C", 8, dtype, "uniform", 0), 0, world)
    for extra in CROWD_EXTRAS:
        crowd = parts_of(("C", 8, dtype, "crowd", extra), 0, world)
        if any(len(c[g]) > halo_capacity(len(u[g])) for u, c in zip(uni, crowd) for g in ("glo", "ghi")):
            return extra
    raise AssertionError("no crowd outgrows a message")


# ------------------------------------------------------------------------------------------------------ the plan


class Caps:
    """The capacities of a rank's two received messages as nl_make_list_distributed negotiates them: with the first
    build, and again for a message whose layer outgrew it."""

    def __init__(self):
        self.neg = [None, None]

    def n_est(self, n_owned, n_lo, n_hi, room):
        """BuildArgs::n_est of the next build (nl_dist.inc), after the negotiation that build would do."""
        for k, c in enumerate((n_lo, n_hi)):
            if self.neg[k] is None or c > halo_capacity(self.neg[k]):
                self.neg[k] = c
        rcap = [halo_capacity(c) for c in self.neg]
        n_upper = min(n_owned + rcap[0] + rcap[1], room)
        return min(n_upper, n_owned + (rcap[0] - 1024) * 4 // 5 + (rcap[1] - 1024) * 4 // 5)


def plan_for(n_est, ncl, dtype, mask, two_level=True):
    """plan_build's thresholds (nl_api.hip) for n_est particles in ncl cells, in the words of build_info()."""
    f32 = np.dtype(dtype) == np.float32
    cap = 1280  # SweepCfg<T>::CAP
    mean = 27.0 * n_est / ncl
    spread = mean + 5.0 * np.sqrt(mean)
    sparse = mean <= 0.85 * cap
    masks, rows_v, nb = sparse, -1, 1
    if f32 and mask == 0 and two_level and not sparse:
        span = mean * 27.0 / 36.0
        for k, (rows_cap, bits) in enumerate(((1279, 16), (1663, 32), (2495, 32))):  # RowsCfg<k>::CAP, bits of its hit word
            if spread <= rows_cap and span + 6.0 * np.sqrt(span) <= 64.0 * bits:
                rows_v = k
                break
    if not sparse:
        nb_ = int((spread + 64.0) / cap) + 1
        if nb_ <= 7:  # FD_NB
            masks, nb = True, nb_
    masks = masks or rows_v >= 0
    small = f32 and mask == 0 and rows_v < 0 and masks and nb == 1 and spread <= cap // 2  # LEAN_SMALL_CAP
    return dict(masks=bool(masks), mask_rows=nb, fine_rows=rows_v + 1, small_cells=int(small))


def first_build_plan(part, box, dtype, mask, room=1 << 30, two_level=True):
    """plan_for a rank's first build on a fresh communicator.  The host-counted path (NL_BINNING=1) plans for the true
    particle count."""
    m = mesh(box)
    n_owned, n_lo, n_hi = len(part["own"]), len(part["glo"]), len(part["ghi"])
    n_est = Caps().n_est(n_owned, n_lo, n_hi, room) if two_level else n_owned + n_lo + n_hi
    return plan_for(n_est, m[0] * m[1] * (part["z_hi"] - part["z_lo"] + 2), dtype, mask, two_level)


# ------------------------------------------------------------------------------------------------------ configurations

F32, F64 = "float32", "float64"


def _plain(key, mask, full, **kw):
    return dict(scenario="plain", key=key, mask=mask, full=full, **kw)


def _cases_one_layer():
    return [_plain(("D", pc, dt, "uniform", 0), mask, full, one_layer=True)
            for pc in (8, 50) for dt in (F32, F64) for mask in (0, 7) for full in (False, True)]


def _cases_two_ranks():
    out = [_plain(("E", 30, dt, "uniform", 0), mask, full) for dt in (F32, F64) for mask in (0, 7) for full in (False, True)]
    out += [_plain(("E", 30, dt, "outside", 0), mask, full, below=bool(mask & 4))
            for dt in (F32, F64) for mask in (0, 7) for full in (False, True)]
    out += [_plain(("E", 1080, dt, "edges", mask), mask, full, below=bool(mask & 4))
            for dt in (F32, F64) for mask in (3, 4) for full in (False, True)]
    return out


def _cases_search_paths():
    return [_plain(("A", pc, dt, "uniform", 0), mask, full, unclipped=True) for pc in (8, 30, 50, 90)
            for dt, mask, full in ((F32, 0, False), (F32, 0, True), (F32, 7, False), (F64, 0, False), (F64, 7, True))]


def _cases_host_counted():
    return [_plain(("B", 30, dt, "uniform", 0), mask, full, two_level=False)
            for dt in (F32, F64) for mask in (0, 7) for full in (False, True)]


TESTS = {  # name: (world, environment, cases)
    "one_layer": (3, None, _cases_one_layer()),
    "two_ranks": (2, None, _cases_two_ranks()),
    "search_paths": (3, None, _cases_search_paths()),
    "empty_rank": (5, None, [dict(scenario="empty_rank", dtype=dt, mask=mask, full=full)
                             for dt in (F32, F64) for mask, full in ((0, False), (7, True))]),
    "rows_boundary": (2, None, [dict(scenario="rows_boundary", dtype=dt, mask=mask, full=full)
                                for dt, mask, full in ((F32, 0, False), (F32, 7, False), (F64, 7, True))]),
    "renegotiation": (2, None, [dict(scenario="renegotiation")]),
    "host_counted": (3, {"NL_BINNING": "1"}, _cases_host_counted()),
    "host_counted_crowd": (2, {"NL_BINNING": "1"}, [dict(scenario="crowd_arrives", dtype=dt, mask=mask, full=full, two_level=False)
                                                    for dt, mask, full in ((F32, 0, False), (F64, 7, True))]),
    "profiled_rank": (2, None, [dict(scenario="profiled", key=("A", 30, F32, "uniform", 0), mask=0, full=False)]),
}


def lists_of_case(case):
    """Every (input key, mask, full list) a case builds: what the CPU test checks the expectations of."""
    s = case["scenario"]
    if s in ("plain", "profiled"):
        return [(case["key"], case["mask"], case["full"])]
    if s == "empty_rank":
        base = ("A", 30, case["dtype"], "vacated", 0)
        return [(base, case["mask"], case["full"]), (("A", 30, case["dtype"], "moved", ("vacated", 0)), case["mask"], case["full"])]
    if s == "rows_boundary":
        return [(("B", 30, case["dtype"], "uniform", 0), case["mask"], case["full"])]
    if s == "crowd_arrives":
        dt = case["dtype"]
        return [(("C", 8, dt, "uniform", 0), case["mask"], case["full"]), (("C", 8, dt, "crowd", crowd_extra(dt)), case["mask"], case["full"])]
    assert s == "renegotiation"
    c64, c32 = ("C", 8, F64, "crowd", crowd_extra(F64)), ("C", 8, F32, "crowd", crowd_extra(F32))
    return [(("C", 8, F64, "uniform", 0), 7, True), (c64, 7, True), (c32, 0, False),
            (("C", 8, F32, "moved", ("crowd", crowd_extra(F32))), 0, False)]


# ------------------------------------------------------------------------------------------------------ one rank


class Rank:
    def __init__(self, rank, world, cases):
        self.rank, self.world = rank, world
        self.msgs, self.records, self.aborted = [], [], False
        n = max(len(get_input(key)) for case in cases for key, _, _ in lists_of_case(case))
        # room for the owned particles and two messages at their capacities (count + 25 % + 1024), whatever the rank
        self.n_max = n + 2 * (1024 + n * 5 // 4) + 64

    def check(self, what, fn, *args):
        """fn(*args); a failure becomes a message and the rank goes on."""
        import traceback

        try:
            return fn(*args)
        except Exception as e:  # (an assertion of check_rows, or anything else the check ran into)
            at = traceback.extract_tb(e.__traceback__)[-1]
            self.msgs.append(f"rank {self.rank}: {what}: {type(e).__name__}: {str(e)[:700]} [{at.name}:{at.lineno}]")
            return None

    def build(self, dn, sync, what, allowed=()):
        """One build on every rank (sync=False: followed by synchronize); returns the ranks' status codes.  A code outside
        `allowed` on any rank ends the remaining configurations on every rank, here."""
        import torch.distributed as dist

        from md_neighbor_list_amd._lib import NLError

        code = 0
        try:
            dn.build(sync=sync)
            if not sync:
                dn.nl.synchronize()
        except NLError as e:
            code = e.code
            if code not in allowed:
                self.msgs.append(f"rank {self.rank}: {what} sync={sync}: {e}")
        except Exception as e:
            code = -1
            self.msgs.append(f"rank {self.rank}: {what} sync={sync}: {type(e).__name__}: {e}")
        flags = [None] * self.world
        dist.all_gather_object(flags, (code, code != 0 and code not in allowed))
        if any(f[1] for f in flags):
            self.aborted = True
            raise Abort()
        return [f[0] for f in flags]

    def new_handle(self, box_name, dtype, mask, full, n_max=None, capacity=None):
        from md_neighbor_list_amd.dist import DistributedNeighList

        nl = make_handle(BOXES[box_name], self.n_max if n_max is None else n_max, dtype, mask, full=full, capacity=capacity)
        return nl, DistributedNeighList(nl, self.rank, self.world, transport="host")


def scatter(dn, key):
    import torch

    dn.scatter(torch.from_numpy(np.array(get_input(key))).cuda(), BOXES[key[0]], RC)


def own_part(dn):
    """The `part` of check_rows for the rows this rank holds."""
    return dict(own=dn.gid_owned.cpu().numpy().astype(np.int64), z_lo=dn.z_lo, z_hi=dn.z_hi)


def check_scatter(R, dn, me, box):
    assert (dn.z_lo, dn.z_hi) == slab.split_layers(mesh(box)[2], R.world)[R.rank] == (me["z_lo"], me["z_hi"]), (dn.z_lo, dn.z_hi)
    assert dn.n_owned == len(me["own"]) and np.array_equal(own_part(dn)["own"], me["own"]), \
        f"scatter keeps {dn.n_owned} particles, the filing rule of the library {len(me['own'])}"


def check_build(nl, dn, me, glob, what, plan):
    """The last build of this rank: ghost counts = the populations of its two neighbour layers, rows = the rows of the
    global list (check_rows), the search path, the two-pass (or atomic-rank) binning.  Returns the checksum."""
    ghosts = dn.ghosts()
    assert ghosts == (len(me["glo"]), len(me["ghi"])), f"{what}: ghosts {ghosts}, layers hold {(len(me['glo']), len(me['ghi']))}"
    got = read_slab(nl)
    cs = check_rows(got, own_part(dn), glob, what)
    assert got["stats"]["cap_row"] == 0, (what, got["stats"])  # (no row buckets: the counts are not the host's)
    assert got["info"]["variant"] == 3 and got["info"]["offset_bits"] == 32 and got["info"]["id_classes"] == 0, (what, got["info"])
    for name, want in (plan or {}).items():
        assert got["info"][name] == want, f"{what}: {name} = {got['info'][name]}, expected {want}; {got['info']}"
    return cs


def build_pair(R, nl, dn, key, mask, full, what, plan=None, me=None):
    """A synchronous, then an asynchronous build of the scattered input `key`, both checked."""
    me = parts_of(key, mask, R.world)[R.rank] if me is None else me
    R.check(f"{what}: scatter", check_scatter, R, dn, me, BOXES[key[0]])
    glob = get_list(key, mask, full)
    for sync in (True, False):
        R.build(dn, sync, what)
        cs = R.check(f"{what} sync={sync}", check_build, nl, dn, me, glob, what, plan(sync) if callable(plan) else plan)
        R.records.append((f"{what} sync={sync}", dn.n_owned, cs, len(glob[0]), list_sum(key, mask, full)))
    return me


def scenario_plain(R, case):
    key, mask, full = case["key"], case["mask"], case["full"]
    box = BOXES[key[0]]
    what = f"{key} mask {mask} {'full' if full else 'half'}"
    nl, dn = R.new_handle(key[0], key[2], mask, full)  # a fresh communicator: capacities negotiated for THIS input
    scatter(dn, key)
    parts = parts_of(key, mask, R.world)
    me = parts[R.rank]
    two_level = case.get("two_level", True)
    plan = expected_plan(30 if key[3] == "edges" else key[1], key[2], mask)
    if not two_level:
        plan = dict(plan, fine_rows=0, masks=True)  # (NL_BINNING=1, as tests/test_slab_paths.py asserts it)

    def before():
        # expected_plan is what the rank's own estimate gives (checked for every case by the CPU test as well)
        assert first_build_plan(me, box, key[2], mask, two_level=two_level) == plan
        if case.get("unclipped"):
            room = len(me["own"]) + 2 * (1024 + max(len(me["glo"]), len(me["ghi"])) * 5 // 4)
            assert R.n_max >= room and dn.q.shape[0] >= room, (R.n_max, dn.q.shape[0], room)
        if case.get("one_layer"):  # both ghost layers are whole ranks: the other two
            assert len(me["glo"]) == len(parts[(R.rank - 1) % 3]["own"]) and len(me["ghi"]) == len(parts[(R.rank + 1) % 3]["own"])
            assert me["z_hi"] - me["z_lo"] == 1
        if case.get("below"):
            # particles less than a cell below z = 0: layer 0 by the reference's truncation, the top layer by the floor
            # the library takes where z is periodic -- the top rank's
            q = get_input(key)
            ms_z = box[2] / mesh(box)[2]
            below = np.flatnonzero((q[:, 2] < 0) & (q[:, 2] > -0.99 * ms_z))
            assert len(below) > 0
            assert (layers_of(q, box, 0)[below] == 0).all() and (layers_of(q, box, mask)[below] == mesh(box)[2] - 1).all()
            mine = np.isin(below, own_part(dn)["own"])
            assert mine.all() if R.rank == R.world - 1 else not mine.any(), f"{int(mine.sum())} of {len(below)} particles below z = 0 are here"

    R.check(f"{what}: setting", before)
    build_pair(R, nl, dn, key, mask, full, what, plan, me)


def scenario_empty_rank(R, case):
    dt, mask, full = case["dtype"], case["mask"], case["full"]
    keys = [k for k, _, _ in lists_of_case(case)]
    box, m = BOXES["A"], mesh(BOXES["A"])
    nl, dn = R.new_handle("A", dt, mask, full)
    caps, seen = Caps(), []
    for rnd, key in enumerate(keys):
        what = f"{key} mask {mask} {'full' if full else 'half'}"
        scatter(dn, key)  # (round 1: the same handle and communicator, every particle moved)
        me = parts_of(key, mask, R.world)[R.rank]
        room = min(R.n_max, int(dn.q.shape[0]))

        def plan(sync, me=me, room=room):
            # a rank's estimate here is far from 30 per cell (an empty neighbour layer, capacities from before the move):
            # the path is the one plan_build's thresholds give for this rank's n_est
            return plan_for(caps.n_est(len(me["own"]), len(me["glo"]), len(me["ghi"]), room), m[0] * m[1] * (me["z_hi"] - me["z_lo"] + 2), dt, mask)

        build_pair(R, nl, dn, key, mask, full, what, plan, me)

        def empty():
            got = read_slab(nl)
            assert dn.n_owned == 0 and len(got["key_pointer"]) == 1 and got["entries"] == 0 and len(got["partners"]) == 0, (dn.n_owned, got["entries"])

        if R.rank == 2 and rnd == 0:
            R.check(f"{what}: the rank without particles", empty)
        seen.append((dn.n_owned, len(me["glo"]), len(me["ghi"])))

    def changed():
        assert seen[0][0] != seen[1][0] and seen[0][1:] != seen[1][1:], seen
        if R.rank == 2:
            assert seen[0][0] == 0 < seen[1][0], seen

    R.check("owned and ghost counts after the move", changed)


def scenario_profiled(R, case):
    """Rank 0 alone profiles its last build, as bench.py does at world > 1 (nl_profile_last_build with the device-side
    ghost counts: a.n = h->n, BuildArgs::dyn set): its rows, ghost counts and checksum stay the oracle's, its peer's are
    untouched, and the next collective build is exact on both."""
    key, mask, full = case["key"], case["mask"], case["full"]
    what = f"{key} mask {mask} {'full' if full else 'half'}"
    nl, dn = R.new_handle(key[0], key[2], mask, full)
    scatter(dn, key)
    me = build_pair(R, nl, dn, key, mask, full, what)
    glob = get_list(key, mask, full)

    def profile():
        ms = nl.profile_last_build(reps=2)
        assert len(ms) == 7 and all(np.isfinite(v) and v >= 0 for v in ms.values()) and ms["total"] > 0, ms

    def record(stage):
        cs = R.check(f"{what}: {stage}", check_build, nl, dn, me, glob, f"{what}: {stage}", None)
        R.records.append((f"{what}: {stage}", dn.n_owned, cs, len(glob[0]), list_sum(key, mask, full)))

    if R.rank == 0:  # (no collective call inside: the peer does not wait for it)
        R.check(f"{what}: profile_last_build on rank 0", profile)
    record("after rank 0 profiled")
    R.build(dn, True, f"{what}: the build after profiling")
    record("the build after profiling")


def exact_rows(t, rows):
    """A buffer of exactly `rows` rows (its own allocation)."""
    return t[:rows].clone()


def scenario_rows_boundary(R, case):
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY

    dt, mask, full = case["dtype"], case["mask"], case["full"]
    key = ("B", 30, dt, "uniform", 0)
    what = f"{key} mask {mask} {'full' if full else 'half'}"
    me = parts_of(key, mask, R.world)[R.rank]
    total = len(me["order"])  # n_owned + ghosts from below + ghosts from above, from the oracle's filing
    nl, dn = R.new_handle("B", dt, mask, full, n_max=total)
    plan = expected_plan(30, dt, mask)
    glob = get_list(key, mask, full)
    # (a) rows for exactly owned + ghosts, in the buffer and in the handle: n_upper is clipped to the true total
    scatter(dn, key)
    dn.q = exact_rows(dn.q, total)
    build_pair(R, nl, dn, key, mask, full, what + " (a) exact room", plan, me)
    # (b) one row fewer on rank 0: refused there (after the exchange: rank 1 builds), counts 0 and 0
    if R.rank == 0:
        dn.q = exact_rows(dn.q, total - 1)
    for sync in (True, False):
        codes = R.build(dn, sync, what + " (b)", allowed=(NL_ERR_CAPACITY,) if R.rank == 0 else ())

        def refused(codes=codes):
            assert codes == [NL_ERR_CAPACITY, 0], codes
            if R.rank == 0:
                assert dn.ghosts() == (0, 0), (dn.n_ghost_lo, dn.n_ghost_hi)

        R.check(f"{what} (b) one row short on rank 0, sync={sync}", refused)
        if R.rank == 1:
            R.check(f"{what} (b) rank 1, sync={sync}", check_build, nl, dn, me, glob, what, plan)
    # (c) the same handle and communicator with the right room again
    scatter(dn, key)
    dn.q = exact_rows(dn.q, total)
    build_pair(R, nl, dn, key, mask, full, what + " (c) room again", plan, me)


def check_outgrown(R, key_u, key_c, mask):
    u, c = parts_of(key_u, mask, R.world), parts_of(key_c, mask, R.world)
    assert any(len(c[r][g]) > halo_capacity(len(u[r][g])) for r in range(R.world) for g in ("glo", "ghi")), "no layer outgrows its message"


def scenario_crowd_arrives(R, case):
    """Capacities negotiated for the uniform part; then the crowd: a synchronous build renegotiates and ends exact."""
    dt, mask, full = case["dtype"], case["mask"], case["full"]
    (key_u, _, _), (key_c, _, _) = lists_of_case(case)
    nl, dn = R.new_handle("C", dt, mask, full)
    scatter(dn, key_u)
    plan = dict(fine_rows=0, masks=True) if not case.get("two_level", True) else None
    build_pair(R, nl, dn, key_u, mask, full, f"{key_u} mask {mask} full {full}", plan)
    R.check("crowd", check_outgrown, R, key_u, key_c, mask)
    scatter(dn, key_c)
    build_pair(R, nl, dn, key_c, mask, full, f"{key_c} mask {mask} full {full}", plan)


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("counts", "key_pointer", "partners")) and a["checksum"] == b["checksum"]


def scenario_renegotiation(R, case):
    import torch

    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY

    (u64, _, _), (c64, _, _), (c32, _, _), (m32, _, _) = lists_of_case(case)
    box = BOXES["C"]
    # 1. fp64, mask 7, full list: capacities negotiated near their floor, then the crowd
    h64, dn = R.new_handle("C", F64, 7, True, capacity=int(get_list(c64, 7, True)[1][-1]))  # (an asynchronous build cannot grow its list)
    scatter(dn, u64)
    build_pair(R, h64, dn, u64, 7, True, "1. uniform part")
    R.check("1. crowd", check_outgrown, R, u64, c64, 7)
    scatter(dn, c64)
    codes = R.build(dn, False, "1. crowd, first build", allowed=(NL_ERR_CAPACITY,))

    def reported():
        assert NL_ERR_CAPACITY in codes, codes

    R.check("1. a layer outgrew its message: NL_ERR_CAPACITY at synchronize", reported)
    build_pair(R, h64, dn, c64, 7, True, "1. crowd, renegotiated")
    part64, rows64 = own_part(dn), read_slab(h64)
    # 2. a second handle on the same communicator: 16-byte elements, all four messages anew
    h32 = make_handle(box, R.n_max, F32, 0, full=False)
    dn.nl = h32
    scatter(dn, c32)
    build_pair(R, h32, dn, c32, 0, False, "2. fp32 handle")

    def first_handle(stage):
        got = read_slab(h64)
        assert same_rows(got, rows64), stage
        check_rows(got, part64, get_list(c64, 7, True), stage)

    R.check("2. the first handle's rows", first_handle, "after the second handle's builds")
    # 3. the same handle and communicator after every particle has moved
    # (nl_set_graph(1) on a distributed build is NOT run here: see the docstring of the test)
    scatter(dn, m32)
    build_pair(R, h32, dn, m32, 0, False, "3. moved particles")
    # 4. the communicator goes, both handles stay
    part32, rows32 = own_part(dn), read_slab(h32)
    del dn  # nl_comm_destroy

    def survivors():
        first_handle("after nl_comm_destroy")
        got = read_slab(h32)
        assert same_rows(got, rows32)
        check_rows(got, part32, get_list(m32, 0, False), "fp32 handle after nl_comm_destroy")
        q = get_input(c32)
        h32.MakeNeighList(torch.from_numpy(np.array(q)).cuda(), len(q))
        check_rows(read_slab(h32), dict(own=np.arange(len(q)), z_lo=0, z_hi=mesh(box)[2]), get_list(c32, 0, False), "whole box")

    R.check("4. handles that outlive their communicator", survivors)


SCENARIOS = dict(plain=scenario_plain, profiled=scenario_profiled, empty_rank=scenario_empty_rank, rows_boundary=scenario_rows_boundary,
                 crowd_arrives=scenario_crowd_arrives, renegotiation=scenario_renegotiation)


def check_records(gathered):
    """Rank 0, per build: the owned counts add up to n and the ranks' checksums to the checksum of the global list."""
    out = []
    for recs in zip(*gathered):
        what, n, want = recs[0][0], recs[0][3], recs[0][4]
        if sum(r[1] for r in recs) != n:
            out.append(f"{what}: the ranks own {[r[1] for r in recs]} particles of {n}")
        if all(r[2] is not None for r in recs) and sum(r[2] for r in recs) & MASK64 != want:
            out.append(f"{what}: the ranks' checksums do not add up to the global list's")
    return out


def worker(rank, world, port, cases, env, ret):
    import traceback
    from datetime import timedelta

    os.environ.update(env or {})  # (before the library is loaded)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    try:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
        R = Rank(rank, world, cases)
        failures, builds = [], 0
        for case in cases:
            if not R.aborted:
                try:
                    SCENARIOS[case["scenario"]](R, case)
                except Abort:
                    pass
            gathered = [None] * world
            dist.all_gather_object(gathered, (R.msgs, R.records))
            if rank == 0:
                for msgs, _ in gathered:
                    failures += msgs
                if not R.aborted:
                    failures += check_records([g[1] for g in gathered])
                builds += len(R.records)
            R.msgs, R.records = [], []
        if rank == 0:
            ret.put(("fail", failures) if failures or R.aborted else ("ok", len(cases), builds))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover  (a fault of the worker itself: the peers run into their time limit)
        ret.put(("fail", [f"rank {rank}: {traceback.format_exc()}"]))
        raise


def run(world, cases, env=None, timeout=180):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, cases, env, ret)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = ret.get(timeout=timeout)
    finally:
        for p in procs:
            p.join(timeout=20)
            if p.is_alive():
                p.terminate()
    assert res[0] == "ok", "\n".join(str(m) for m in res[1])
    return res

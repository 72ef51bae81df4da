"""Every entry point that takes a stream, called on a caller's non-blocking stream that is held back by a delay.

include/nl_hip.h promises that a call is ordered after everything already queued on the stream it is given, and nothing
else.  On the null stream, which the rest of the suite uses, a launch, memset or copy on the wrong stream cannot show: the
null stream orders itself against everything.  Here the stream is a torch side stream (non-blocking) whose first work is a
delay; the inputs are copied into their tensors behind it, and until then the tensors hold a decoy (tests/stream_util.py).
Whatever the library issues elsewhere runs at once and reads the decoy, or an intermediate that is not written yet.

Every comparison reuses a reference and a bound the suite already has: the oracle's list (list_of, check_rows of
tests/test_slab_paths.py; want, replay, check_list of tests/test_update_paths.py), the float64 sums and bounds of the consumer
families (the Consumer records of their test files, check_lj, check_virial, check_hist), pair_vectors_ref, remove_pairs and
type_filter.  The non-vacuity assertions (Held.assert_held) are made in every GPU test: before the first library call of a
sequence, and behind the last one wherever the sequence only enqueues on a handle that was warmed.

Sections: the harness and its teeth; A builds on every path; B nl_update_list chains; C the consumers (enqueued, blocking
from another stream, the shared scratch under a caller's fence); D getters, nl_resort, the setters whose arrays come from
the caller's stream; E slab builds in two parts; F two handles on two streams.
"""
import functools

import numpy as np
import pytest

from tests import test_update_paths as upd  # (a module: its tests are not collected here)
from tests import util_coul_excl as ux
from tests import util_coulomb as uc
from tests.consumer_util import N, R_MAX, R_MIN, RCF, _handle, _lj_input, _lj_moved, _lj_moved_pairs, _lj_pairs, _lj_par, _tdt
from tests.consumer_util import _table_input, _table_moved
from tests.hist_util import check_hist, hist_r2
from tests.stream_util import device, held_stream, rolled, unrolled_ids
from tests.test_slab_paths import (BOXES, DECOMPS, FORCED, LIST_QUIET_BUILDS, RC, _canonical, _symmetrised, check_rows, expected_plan,
                                   global_list, list_of, make_handle, make_input, mix_sum, read_slab, relabelled, slab_parts)
from tests.util import LJ_BOXES, LJ_C, check_lj, lj_pairs, lj_reference, lj_unit
from tests.virial_util import check_virial

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


def _torch():
    import torch

    return torch


def _po():
    from oracle import pyoracle as po

    return po


# ----------------------------------------------------------------------------------------- the consumer families
@functools.lru_cache(maxsize=None)
def family(name):
    """(Consumer record, bound constant of its forces, reference of other positions) of a table-driven family."""
    if name == "table":
        from tests import test_pair_table as m
        from tests.util_table import TABLE_C

        return m.TABLE, TABLE_C, lambda q, box, kind, pairs, chg: m._refs(q, box, kind, pairs)
    if name == "eam":
        from tests import test_eam as m
        from tests.util_eam import EAM_C

        return m.EAM, EAM_C, lambda q, box, kind, pairs, chg: m._refs(q, box, kind, pairs)
    if name == "sw":
        from tests import test_sw as m
        from tests.util_sw import SW_C

        return m.SW, SW_C, lambda q, box, kind, pairs, chg: m._refs(q, box, kind, pairs)
    if name == "coul":
        from tests import test_coulomb as m

        def other(q, box, kind, pairs, chg):
            mo = uc.model(kind)
            mo = uc.Model(mo.F, mo.U, mo.r_min, mo.r_max, mo.K, mo.C, mo.r_min_c, mo.r_max_c, chg, mo.types, mo.rc_ab)
            return uc.coul_reference(q, *LJ_BOXES[box], mo, pairs)

        return m.COUL, uc.COUL_C, other
    assert name == "coulx"
    from tests import test_coul_excl as m

    def other(q, box, kind, pairs, chg):
        return ux.excl_reference(q, *LJ_BOXES[box], *ux.excl_tab(), R_MIN, R_MAX, chg, ux.topology(kind.split("/")[0], box)[1])

    return m.COULX, ux.COULX_C, other


# (family, box, kind, list kinds): the boxes and kinds of each family's test_reuse_within_the_skin
FAMILY_CASES = [("table", "xyz", "morse", (False, True)), ("table", "tilt", "typed3", (False, True)),
                ("eam", "xyz", "one", (False, True)), ("eam", "tilt", "three", (False, True)),
                ("sw", "xyz", "one", (True,)), ("sw", "tilt", "three", (True,)),
                ("coul", "xyz", "salt", (False, True)), ("coul", "tilt", "typed3", (False, True)),
                ("coulx", "xyz", "chains/xyz", (False, True)), ("coulx", "tilt", "mixed/tilt", (False, True))]
FAMILY_IDS = [f"{f}-{b}-{k.split('/')[0]}" for f, b, k, _ in FAMILY_CASES]
LJ_CASES = [("xyz", "scalar"), ("tilt", "typed3")]
RC_LIST, SKIN = 2.9, 0.4  # tests.consumer_contract.reuse_within_the_skin


def _forces_of(ref):
    """(want[n, 4], S[n, 4]) of a family's reference, whichever layout it has."""
    return (ref["want"], ref["S"]) if isinstance(ref, dict) else ref[0]


def _charges(family_name, kind):
    """The charges a family's set() gives the handle, None for a family without."""
    if family_name == "coul":
        return uc.charges(kind)
    return uc.charges("salt") if family_name == "coulx" else None


# ------------------------------------------------------------------------------------------------------------ CPU
BUILD_KEYS = [(b, d, t, "uniform", 0) for b in "AB" for d in (8, 30, 50, 90) for t in ("float32", "float64")]
CROWD = ("C", 8, "float32", "crowd", 1300)
SPARSE = ("C", 8, "float32", "uniform", 0)


def decoy_list(q, box, mask, full):
    """(counts, key_pointer, partners) of the decoy's list, made from the wanted list alone: rolled(q) is q under the ids
    unrolled_ids, so its list is the wanted one relabelled (a pair sits in the row of the smaller new id) with the rows
    moved to their new places."""
    n = len(q)
    new_id = unrolled_ids(n)
    c, _, vals = relabelled(list_of(q, box, mask, False), new_id, full)
    rows = new_id[np.repeat(np.arange(n, dtype=np.int64), c)]
    order = np.lexsort((vals, rows))
    cnt = np.bincount(rows, minlength=n)
    return cnt, np.concatenate([[0], np.cumsum(cnt)]), vals[order]


def test_decoy_has_another_list():
    """For every input the GPU tests below use, on the CPU: the oracle's list of the rolled positions is the wanted list
    relabelled and differs from it (other counts, other partners), with the same entry count and the same per-cell counts,
    so that a stage which read the decoy shows in the arrays compared and never changes a size.  For the consumers: the
    family's own float64 reference of the decoy (positions and charges rolled, the types where they are) differs from the
    wanted one by more than the family's fp32 bound c u S -- the wider of the two -- on at least 99 % of the particles that
    have a force at all (the excluded-pair term acts on bonded particles only)."""
    po = _po()
    for key in BUILD_KEYS + [CROWD]:
        q, box = make_input(*key), BOXES[key[0]]
        qr = np.array(rolled(q))
        cell, m = po.cells(q, RC, box)
        cell_r, _ = po.cells(qr, RC, box)
        ncell = int(m[0] * m[1] * m[2])
        assert np.array_equal(np.bincount(cell, minlength=ncell), np.bincount(cell_r, minlength=ncell)), key
        for mask in (0, 7) if key[3] == "uniform" else (0,):
            for full in (False, True) if key[1] == 30 else (False,):  # (the full list follows from the half list)
                want, dec = global_list(key, mask, full), list_of(qr, box, mask, full)
                made = decoy_list(q, box, mask, full)
                assert all(np.array_equal(a, b) for a, b in zip(dec, made)), (key, mask, full)
                assert dec[1][-1] == want[1][-1] and (dec[0] != want[0]).any(), (key, mask, full)
                assert not np.array_equal(dec[2], want[2]), (key, mask, full)
    # the consumers: the moved lattice of the enqueued calls, and the lattice in the box (xyz) or drifted (tilt) of the blocking ones
    for fam, box, kind, _ in FAMILY_CASES:
        d, c, other = family(fam)
        box6, mask = LJ_BOXES[box]
        chg = _charges(fam, kind)
        for q1, want in ((_table_moved(box)[0], d.moved_ref(box, kind)), (_table_input(box, box == "tilt"), d.ref(box, box == "tilt", kind))):
            qr = np.array(rolled(q1))
            dec = other(qr, box, kind, lj_pairs(qr, box6, mask, R_MAX * (1 + 2.0 ** -16)), None if chg is None else np.array(rolled(chg)))
            _assert_other_forces(_forces_of(dec)[0], *_forces_of(want), c, (fam, box, kind))
    for box, par in LJ_CASES + [("open", "scalar")]:  # (open, and xyz in the box: the two handles on two streams)
        box6, mask = LJ_BOXES[box]
        types, _, eps, sig, rcf = _lj_par(par, RC_LIST)
        for q1, pairs in ((_lj_moved(box), _lj_moved_pairs(box)), (_lj_input(box, box == "tilt"), _lj_pairs(box, box == "tilt"))):
            qr = np.array(rolled(q1))
            dec, _ = lj_reference(qr, box6, mask, eps, sig, rcf, types=types, pairs=lj_pairs(qr, box6, mask, RCF))
            want, S = lj_reference(q1, box6, mask, eps, sig, rcf, types=types, pairs=pairs)
            _assert_other_forces(dec, want, S, LJ_C, ("lj", box, par))
        q1 = _lj_moved(box)
        qr = np.array(rolled(q1))
        # the histogram counts distances: rolled positions alone have the wanted histogram, rolled against fixed types have not
        if types is not None:
            h_want = hist_r2(lj_pairs(q1, box6, mask, 2.6), N, types, 3, rc_ab=_lj_par(par, RC_LIST)[1])
            h_dec = hist_r2(lj_pairs(qr, box6, mask, 2.6), N, types, 3, rc_ab=_lj_par(par, RC_LIST)[1])
            assert any(len(a) != len(b) for a, b in zip(h_want, h_dec)), (box, par)
    _the_other_decoys()


def _the_other_decoys():
    """The decoys that are not a lattice or a uniform box rolled: each gives another result than the wanted input."""
    from tests.test_exclusions import mixed_pairs, remove_pairs, table_csr
    from tests.test_slab_paths import take_rows
    from tests.test_type_cutoffs import seeded_types, type_filter

    po = _po()
    # the lattices of the two handles, at the list's cut-off: other counts, the same total
    for box in ("xyz", "open"):
        box6, mask = LJ_BOXES[box]
        q = np.ascontiguousarray(_lj_input(box, False))
        build = po.build_pbc if mask else po.build
        a, b = build(q, RC_LIST, box6[:3]), build(np.array(rolled(q)), RC_LIST, box6[:3])
        assert a.npairs == b.npairs and (np.diff(a.key_pointer) != np.diff(b.key_pointer)).any(), box
    # the second build on another stream: reversed positions and their decoy, three different lists
    for dtype in ("float32", "float64"):
        key = ("A", 30, dtype, "uniform", 0)
        q, box = make_input(*key), BOXES["A"]
        q2 = np.ascontiguousarray(q[::-1])
        for mask, full in ((0, False), (7, True)):
            one, two, dec = global_list(key, mask, full), list_of(q2, box, mask, full), list_of(np.array(rolled(q2)), box, mask, full)
            assert one[1][-1] == two[1][-1] == dec[1][-1] and (one[0] != two[0]).any() and (dec[0] != two[0]).any(), (dtype, mask, full)
    # the update chains: what the tensor holds before the chain (step 4) has another list than step 0, and than the last snapshot (step 3)
    for case in CHAINS:
        for full in (False, True):
            w = [upd.want(case["key"], case["mask"], full, step)[0] for step in (0, 3, 4)]
            assert (w[2] != w[0]).any() and (w[2] != w[1]).any() and (w[0] != w[1]).any(), case["name"]
    # the slab build in two parts: the rows rolled within the owned particles and within either ghost layer, under the same ids
    box_name, layers = DECOMPS["B1"]
    for dtype in ("float32", "float64"):
        key = (box_name, 30, dtype, "uniform", 0)
        q, box = make_input(*key), BOXES[box_name]
        glob = global_list(key, 0, False)
        for part in slab_parts(q, box, RC, layers):
            order, n_own, n_lo = part["order"], len(part["own"]), len(part["glo"])
            moved = np.array(q)
            moved[order] = _rolled_within(np.array(q[order]), (0, n_own, n_own + n_lo, len(order)))
            cell, m = po.cells(q, RC, box)
            cell_m, _ = po.cells(moved, RC, box)
            assert np.array_equal(np.sort(cell[order] // (m[0] * m[1])), np.sort(cell_m[order] // (m[0] * m[1])))  # (every layer keeps its count)
            want_c, want_l = take_rows(glob, part["own"])
            dec_c, dec_l = take_rows(list_of(moved, box, 0, False), part["own"])
            assert (want_c != dec_c).any() and not np.array_equal(want_l, dec_l), (dtype, part["z_lo"])
    # the setters and the re-sort: an exclusion table with every index moved up by one, types and arrays rolled
    for box_name in "AB":
        key = (box_name, 30, "float32", "uniform", 0)
        q, box = make_input(*key), BOXES[box_name]
        n = len(q)
        _, kp0, lst0 = global_list(key, 0, False)
        pairs = mixed_pairs(kp0, lst0, n, 51 if box_name == "A" else 41)
        shifted = _shifted_pairs(pairs, n)
        assert len(table_csr(pairs, n)[1]) == len(table_csr(shifted, n)[1]) and not np.array_equal(table_csr(pairs, n)[1], table_csr(shifted, n)[1])
        assert not np.array_equal(remove_pairs(kp0, lst0, pairs)[0], remove_pairs(kp0, lst0, shifted)[0])
        types, rcm = seeded_types(n, 3, 61 if box_name == "A" else 42, RC)
        a = type_filter(kp0, lst0, q, RC, box, 0, np.float32, types, rcm)
        b = type_filter(kp0, lst0, q, RC, box, 0, np.float32, np.array(rolled(types)), rcm)
        assert not np.array_equal(a[0], b[0]), box_name


def _assert_other_forces(dec, want, S, c, what):
    acts = (S > 0).any(axis=1)
    differs = ~(np.abs(dec - want) <= c * lj_unit(np.float32) * S).all(axis=1)
    assert acts.sum() > N // 2 and differs[acts].mean() >= 0.99, (what, int(acts.sum()), float(differs[acts].mean()))


# ------------------------------------------------------------------------------------------------- the harness
@gpu
def test_harness_sees_an_off_stream_read():
    """With the stream held and the copy of the positions queued behind the delay, a copy of the positions tensor on the
    default stream returns the decoy: the side stream does not wait for the null stream or the null stream for it, and the
    delay outlasts the enqueue.  Once the stream has drained the tensor holds the wanted positions."""
    torch = _torch()
    q = make_input("A", 30, "float32")
    src, dec = device(q), device(rolled(q))
    qd = dec.clone()
    seen = torch.zeros_like(qd)
    seen.copy_(src)  # (the copy kernel is loaded and `seen` allocated before the stream is held)
    default = torch.cuda.default_stream()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        with torch.cuda.stream(default):
            seen.copy_(qd)  # (a device copy on the null stream)
            default.synchronize()
        h.assert_held("an off-stream read")
    assert torch.equal(seen, dec) and not torch.equal(seen, src)
    assert torch.equal(qd, src)


# ------------------------------------------------------------------------------------------------------ A: builds
def held_build(nl, qd, src, sync, label=None, delay_ms=None, settle=True):
    """MakeNeighList(qd) on a held stream, the positions copied behind the delay.  label: the handle is warm and the build
    asynchronous, so the call only enqueues."""
    with held_stream(delay_ms, settle=settle) as h:
        h.copy(qd, src)
        h.assert_held()
        nl.MakeNeighList(qd, sync=sync)
        if label is not None:
            h.assert_held(label)
    if not sync:
        nl.synchronize()


def check_whole(nl, glob, what, expect=None, wide=False):
    """The handle's list == (counts, key_pointer, per-row ascending partners) of the oracle, with the entry counts and the
    checksum of nl_hip.h; build_info() / build_stats() say what `expect` says.  Returns read_slab's dict."""
    got = read_slab(nl, wide)
    cnt, kp, lst = glob
    bad = np.flatnonzero(got["counts"] != cnt)
    assert not len(bad), f"{what}: row {bad[0]} has {got['counts'][bad[0]]} partners, the oracle {cnt[bad[0]]}; {len(bad)} rows differ; {got['info']}"
    assert np.array_equal(got["key_pointer"], kp), what
    if not np.array_equal(got["partners"], lst):
        k = int(np.flatnonzero(got["partners"] != lst)[0])
        r = int(np.searchsorted(kp, k, side="right") - 1)
        raise AssertionError(f"{what}: row {r}: got {got['partners'][kp[r]:kp[r + 1]]}, the oracle {lst[kp[r]:kp[r + 1]]}; {got['info']}")
    total = int(kp[-1])
    assert got["entries"] == total and got["checksum_entries"] == total, (what, got["entries"], total)
    assert got["half_pairs"] == (total // 2 if nl.full_list else total), what
    assert got["checksum"] == mix_sum(np.arange(len(cnt)), cnt, lst), what
    for name, w in (expect or {}).items():
        have = got["info"][name] if name in got["info"] else got["stats"][name]
        assert w(have) if callable(w) else have == w, (what, name, have, got["info"], got["stats"])
    return got


BUILD_ROWS = ([(env, "B", d, dts, masks, expect) for env, d, dts, masks, expect in FORCED] +
              [({}, b, d, ("float32", "float64"), (0, 7), None) for b in "AB" for d in (8, 30, 50, 90)])
BUILD_IDS = ["-".join([f"{k}={v}" for k, v in r[0].items()] + [f"{r[1]}{r[2]}"]) for r in BUILD_ROWS]


@gpu
@pytest.mark.parametrize("row", BUILD_ROWS, ids=BUILD_IDS)
def test_builds_on_a_held_stream(row, monkeypatch):
    """Every row of FORCED (box B) and the default plan at 8, 30, 50 and 90 per cell (boxes A and B), masks 0 and 7, both
    dtypes where the row allows, half and full.  Per configuration three builds, each with the positions behind the delay: a
    fresh handle's synchronous build (every buffer is allocated and zeroed inside the call); the same handle, warm, asynchronous
    (the call only enqueues); a fresh handle's asynchronous build.  Exact against the oracle, on the path the row names."""
    env, box_name, per_cell, dtypes, masks, expect0 = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    widths = (True, False) if env.get("NL_OFFSET_WIDTH") == "64" else (False,)
    box = BOXES[box_name]
    for dtype in dtypes:
        key = (box_name, per_cell, dtype, "uniform", 0)
        q = make_input(*key)
        src, dec = device(q), device(rolled(q))
        qd = dec.clone()
        for mask in masks:
            expect = expect0 if expect0 is not None else dict(expected_plan(per_cell, dtype, mask), variant=3, offset_bits=32)
            for full in (False, True):
                glob = global_list(key, mask, full)
                what = (env, box_name, per_cell, dtype, mask, full)
                nl = make_handle(box, len(q), dtype, mask, full)
                fresh = make_handle(box, len(q), dtype, mask, full, capacity=int(glob[1][-1]))
                for handle, sync, label in ((nl, True, None), (nl, False, f"build {what}"), (fresh, False, None)):
                    qd.copy_(dec)
                    held_build(handle, qd, src, sync, label)
                    for wide in widths:
                        check_whole(handle, glob, (what, sync, label), expect, wide)


@gpu
@pytest.mark.parametrize("dtype,mask", [("float32", 0), ("float64", 7)])
def test_a_grown_list_is_refilled_on_a_held_stream(dtype, mask):
    """A capacity of 1000 entries: the synchronous build finds its list too short, grows it and runs the fill again
    (finish()'s growth branch), the positions behind the delay all the while."""
    key = ("B", 30, dtype, "uniform", 0)
    q = make_input(*key)
    src, dec = device(q), device(rolled(q))
    for full in (False, True):
        glob = global_list(key, mask, full)
        assert glob[1][-1] > 50000
        nl = make_handle(BOXES["B"], len(q), dtype, mask, full, capacity=1000)
        qd = dec.clone()
        held_build(nl, qd, src, True)
        check_whole(nl, glob, ("grown", dtype, mask, full), expected_plan(30, dtype, mask))


@gpu
def test_a_build_that_runs_again_on_a_held_stream():
    """The crowd of tests/test_slab_paths.py (test_a_crowd_across_a_cut) on a handle that six sparse builds have made leave
    the launches for cells beyond the LDS buffer out: the build is incomplete and runs again (run_again()), once, when the
    host waits for it; the positions are behind the delay.  The next build is exact without another run."""
    box = BOXES["C"]
    q0, q1 = make_input(*SPARSE), make_input(*CROWD)
    glob = global_list(CROWD, 0, False)
    nl = make_handle(box, len(q1), "float32", capacity=int(glob[1][-1]))
    q0d = device(q0)
    for _ in range(LIST_QUIET_BUILDS + 2):
        nl.MakeNeighList(q0d)
    st = nl.build_stats()
    assert not st["list_launched"] and st["list_reruns"] == 0 and st["row_overflow_reruns"] == 0, st
    check_whole(nl, global_list(SPARSE, 0, False), "sparse")
    src, dec = device(q1), device(rolled(q1))
    qd = dec.clone()
    held_build(nl, qd, src, False)
    got = check_whole(nl, glob, "crowd")
    assert got["stats"]["list_reruns"] + got["stats"]["row_overflow_reruns"] == 1 and got["stats"]["list_launched"], got["stats"]
    assert (upd.stencil_streams(q1, upd.whole(q1, box), box) > got["info"]["lds_batch"]).any()
    qd.copy_(dec)
    held_build(nl, qd, src, True)
    got = check_whole(nl, glob, "crowd, again")
    assert got["stats"]["list_reruns"] + got["stats"]["row_overflow_reruns"] == 1, got["stats"]


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_second_build_on_another_stream(dtype):
    """A build on stream 1, then one of other positions on stream 2 with no host wait in between: the library waits for
    stream 1 on the host (the last_stream != stream branch) before it enqueues on stream 2, and the second list is exact.
    Stream 1 is held for nine times as long as stream 2: without that wait the second build would run first and the first would
    overwrite it once its delay is over -- both streams have drained before the list is read.  That the call has waited is
    asserted: stream 1's inputs have arrived when it returns.  (Stream 2 is held when the call begins; whether it still is
    when the call returns depends on whether the runtime gives the two streams one hardware queue, where the second delay
    starts behind the first.)"""
    key = ("A", 30, dtype, "uniform", 0)
    q = make_input(*key)
    q2 = np.ascontiguousarray(q[::-1])
    box = BOXES["A"]
    for mask, full in ((0, False), (7, True)):
        glob1, glob2 = global_list(key, mask, full), list_of(q2, box, mask, full)
        assert not np.array_equal(glob1[0], glob2[0])
        nl = make_handle(box, len(q), dtype, mask, full, capacity=int(glob2[1][-1]))
        qd1, qd2 = device(rolled(q)), device(rolled(q2))
        src1, src2 = device(q), device(q2)
        nl.MakeNeighList(qd1)  # (warm)
        with held_stream(450.0) as h1:
            h1.copy(qd1, src1)
            h1.assert_held()
            nl.MakeNeighList(qd1, sync=False)
            h1.assert_held(f"first of two builds {dtype}")
            with held_stream(50.0, settle=False) as h2:  # (at most 7 streams passed over: 350 ms of stream 1's 450)
                h2.copy(qd2, src2)
                h2.assert_held()
                h1.assert_held()  # (the first build is still pending on the device when the second call begins)
                nl.MakeNeighList(qd2, sync=False)
                assert h1.event.query(), "the second build was enqueued while the first was pending on another stream"
        nl.synchronize()
        check_whole(nl, glob2, ("second stream", dtype, mask, full))


# --------------------------------------------------------------------------------------------- B: update chains
def _pick(name):
    (c,) = [c for c in upd.CASES if c["name"] == name]
    return c


CHAINS = [_pick(n) for n in ("B30-32-m0", "B30-64-m7", "NL_SWEEP_VARIANT=1-B30-32-m0", "NL_SWEEP_VARIANT=1-B30-64-m7",
                             "NL_BINNING=1-B30-32-m7", "NL_BINNING=1-B30-64-m0")]


@gpu
@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
@pytest.mark.parametrize("case", CHAINS, ids=[c["name"] for c in CHAINS])
def test_update_chain_on_a_held_stream(case, graph, monkeypatch):
    """The five-step trajectory of tests/test_update_paths.py enqueued behind one delay, each step a copy of the next
    positions and an update; the decoy is what the tensor holds: the last step's positions.  The handle is warm (the whole
    chain has run once; nl_set_skin then forces the first update's build again without touching the graph), so the
    sequence only enqueues.  The updates decide as replay() says and the list is the oracle's of the last snapshot.  graph:
    the library's own graph (nl_set_graph), captured on its private stream, launched on the caller's."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    key, mask = case["key"], case["mask"]
    seq = upd.trajectory(key)[0]
    built, snaps = upd.replay(seq, BOXES[key[0]], mask)
    nl = make_handle(BOXES[key[0]], len(seq[0]), key[2], mask, graph=graph, capacity=upd.capacity_for(case))
    nl.set_skin(upd.SKIN)
    dev = device(np.stack(seq))
    qd = dev[-1].clone()
    for kind in case["kinds"]:
        what = (case["name"], kind, graph)
        nl.set_full_list(kind == "full")
        for k in range(len(seq)):
            qd.copy_(dev[k])
            nl.update(qd)
        nl.synchronize()
        nl.set_skin(upd.SKIN)
        before = nl.update_stats()
        with held_stream() as h:
            for k in range(len(seq)):
                h.copy(qd, dev[k])
                if k == 0:
                    h.assert_held()
                nl.update(qd)
            h.assert_held(f"update chain {what}")
        nl.synchronize()
        after = nl.update_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (len(seq), sum(built)), (what, before, after, built)
        got = upd.check_list(nl, key, mask, snaps[-1], what)
        upd.check_path(got, case, what)


# -------------------------------------------------------------------------------------------------- C: consumers
def _family_handle(d, box, kind, full, dtype):
    nl = _handle(box, dtype, full, RC_LIST)
    nl.set_skin(SKIN)
    nl.Initialize(N)
    d.set(nl, kind, RC_LIST)
    return nl


def _decoy_charges(nl):
    """(the handle's charge tensor, now holding the decoy; the wanted charges) or (None, None)."""
    cd = nl._charges
    if cd is None:
        return None, None
    csrc = cd.clone()
    cd.copy_(_torch().roll(csrc, -1))
    return cd, csrc


def _outputs(dtype):
    torch = _torch()
    return (torch.full((N, 4), -1.0, dtype=_tdt(dtype), device="cuda"), torch.full((8,), -1.0, dtype=torch.float64, device="cuda"))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam,box,kind,kinds", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_enqueued_on_a_held_stream(fam, box, kind, kinds, dtype):
    """Pair table, EAM (with its densities), Stillinger-Weber, Coulomb and the excluded-pair term: behind the delay the moved
    positions (and the charges) are copied, then update, forces and totals are enqueued into preallocated outputs.  The
    handle has built the decoy and run every call once, so nothing allocates and the sequence only enqueues; the decoy lies
    further than skin / 2 from the moved positions, so the update's build runs, on the device's own decision."""
    torch = _torch()
    d = family(fam)[0]
    q1 = _table_moved(box)[0]
    src, dec = device(q1, dtype), device(rolled(q1), dtype)
    for full in kinds:
        nl = _family_handle(d, box, kind, full, dtype)
        forces, virial = getattr(nl, d.forces), getattr(nl, d.virial)
        qd = dec.clone()
        cd, csrc = _decoy_charges(nl)
        fd, wd = _outputs(dtype)
        nl.update(qd, sync=True)
        forces(qd), virial(qd), forces(qd, wait=False, out=fd), virial(qd, wait=False, out=wd), d.extra(nl)
        torch.cuda.synchronize()
        fd.fill_(-1.0), wd.fill_(-1.0)
        before = nl.update_stats()
        with held_stream() as h:
            h.copy(qd, src)
            if cd is not None:
                h.copy(cd, csrc)
            h.assert_held()
            nl.update(qd)
            forces(qd, wait=False, out=fd)
            virial(qd, wait=False, out=wd)
            h.assert_held(f"{fam} {box} {kind} {full} {np.dtype(dtype).name}")
        torch.cuda.synchronize()
        assert nl.update_stats() == (before[0] + 1, before[1] + 1)
        d.check(fd, wd, d.extra(nl), d.moved_ref(box, kind), dtype)


def fenced_totals(nl, virial, qd, src, dec, cd, csrc, label):
    """The totals' scratch on two streams under the caller's fence, in the form that depends on it.  The list is built from
    the wanted positions and synchronised, so no call below waits for anything; the tensors then hold the decoy again.  On
    the held stream: the copies behind the delay, the totals enqueued into w1, an event.  On a second stream: a wait for that
    event -- all that orders it behind the copies and behind the first call's use of the scratch -- and the totals enqueued
    into w2.  The host has only enqueued: the held stream is still held behind the last call.  Returns (w1, w2)."""
    torch = _torch()
    qd.copy_(src)
    if cd is not None:
        cd.copy_(csrc)
    nl.update(qd, sync=True)
    w1 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    w2 = w1.clone()
    virial(qd, wait=False, out=w1)
    torch.cuda.synchronize()
    w1.fill_(-1.0)
    qd.copy_(dec)
    if cd is not None:
        cd.copy_(torch.roll(csrc, -1))
    other = torch.cuda.Stream()
    with held_stream() as h:
        h.copy(qd, src)
        if cd is not None:
            h.copy(cd, csrc)
        h.assert_held()
        virial(qd, wait=False, out=w1)
        fence = torch.cuda.Event()
        fence.record(h.stream)
        with torch.cuda.stream(other):
            other.wait_event(fence)
            virial(qd, wait=False, out=w2)
        h.assert_held(label)
    torch.cuda.synchronize()
    return w1, w2


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam,box,kind,kinds", FAMILY_CASES, ids=FAMILY_IDS)
def test_family_blocking_from_another_stream(fam, box, kind, kinds, dtype):
    """An asynchronous build on the held stream, then the blocking calls with another stream current -- the default stream,
    and a second side stream: they wait for the build first (include/nl_hip.h), so they read the list of the wanted
    positions.  Boxes: xyz in the box, tilt drifted.  Then the shared scratch (the answer to the question of who orders two
    calls of the totals on two streams: the caller): fenced_totals."""
    torch = _torch()
    d = family(fam)[0]
    drift = box == "tilt"
    q = _table_input(box, drift)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    ref = d.ref(box, drift, kind)
    for full in kinds:
        nl = _family_handle(d, box, kind, full, dtype)
        forces, virial = getattr(nl, d.forces), getattr(nl, d.virial)
        qd = dec.clone()
        cd, csrc = _decoy_charges(nl)
        nl.MakeNeighList(qd)  # (grows the list: an asynchronous build cannot)
        forces(qd), virial(qd)
        for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
            qd.copy_(dec)
            if cd is not None:
                cd.copy_(torch.roll(csrc, -1))
            with held_stream() as h:
                h.copy(qd, src)
                if cd is not None:
                    h.copy(cd, csrc)
                h.assert_held()
                nl.MakeNeighList(qd, sync=False)
                h.assert_held(f"asynchronous build {fam} {box} {full}")
                with torch.cuda.stream(other):
                    f = forces(qd)
                    x = d.extra(nl)
                    w = virial(qd)
                    other.synchronize()
            d.check(f, w, x, ref, dtype)
        w1, w2 = fenced_totals(nl, virial, qd, src, dec, cd, csrc, f"totals {fam} {box} {full}")
        f = forces(qd)
        d.check(f, w1, d.extra(nl), ref, dtype)
        d.check(f, w2, d.extra(nl), ref, dtype)


@functools.lru_cache(maxsize=None)
def _filtered_moved_ref(box, topo):
    """uc.moved_ref of the salt model over the pairs the list keeps once the topology's pairs are excluded."""
    box6, mask = LJ_BOXES[box]
    q, (I, J, dd, raw) = _table_moved(box)
    unique = ux.topology(topo, box)[1]
    keys = np.concatenate([unique[:, 0] * N + unique[:, 1], unique[:, 1] * N + unique[:, 0]])
    keep = ~np.isin(I * N + J, keys)
    return uc.coul_reference(q, box6, mask, uc.model("salt"), (I[keep], J[keep], dd[keep], raw[keep]))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,topo", [("xyz", "chains"), ("tilt", "mixed")])
def test_excluded_term_added_behind_coul_forces_on_a_held_stream(box, topo, dtype):
    """coul_forces into a buffer and coul_excl_forces(add=True) into the same buffer, both enqueued behind the update, the
    positions and charges behind the delay (full list: both calls are reproducible).  The buffer is, bit for bit, the sum in
    the position type of what the two blocking calls return afterwards, and those are within their bounds of the float64
    references of the filtered list and of the excluded pairs."""
    torch = _torch()
    COUL, COULX = family("coul")[0], family("coulx")[0]
    q1 = _table_moved(box)[0]
    src, dec = device(q1, dtype), device(rolled(q1), dtype)
    nl = _family_handle(COUL, box, "salt", True, dtype)
    COULX.set(nl, f"{topo}/{box}")
    qd = dec.clone()
    cd, csrc = _decoy_charges(nl)
    fd = _outputs(dtype)[0]
    nl.update(qd, sync=True)
    nl.coul_forces(qd, wait=False, out=fd), nl.coul_excl_forces(qd, wait=False, out=fd, add=True)
    torch.cuda.synchronize()
    with held_stream() as h:
        h.copy(qd, src)
        h.copy(cd, csrc)
        h.assert_held()
        nl.update(qd)
        nl.coul_forces(qd, wait=False, out=fd)
        nl.coul_excl_forces(qd, wait=False, out=fd, add=True)
        h.assert_held(f"coul + excluded {box} {np.dtype(dtype).name}")
    torch.cuda.synchronize()
    fl, fx = nl.coul_forces(qd), nl.coul_excl_forces(qd)
    assert torch.equal(fd, fl + fx) and not torch.equal(fd, fl)
    (want, S), _ = _filtered_moved_ref(box, topo)
    check_lj(fl.cpu().numpy(), want, S, dtype, c=uc.COUL_C)
    (want, S), _ = ux.moved_ref(box, topo)
    check_lj(fx.cpu().numpy(), want, S, dtype, c=ux.COULX_C)


def _lj_handle(box, par, full, dtype, images=False):
    nl = _handle(box, dtype, full, RC_LIST, images=images)
    nl.set_skin(SKIN)
    nl.Initialize(N)
    types, rc_ab, eps, sig, rcf = _lj_par(par, RC_LIST)
    if types is not None:
        nl.set_type_cutoffs(types, rc_ab)
        nl.set_lj_type_params(eps, sig, rcf)
    return nl


def _lj_calls(nl, par):
    """(forces, totals) of a parameter set, as callables (qd, wait, out)."""
    if par == "scalar":
        return (lambda qd, **kw: nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF, **kw), lambda qd, **kw: nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF, **kw))
    return nl.lj_forces_typed, nl.lj_virial_typed


@functools.lru_cache(maxsize=None)
def _lj_refs(box, par, moved):
    """((want, S) of the forces, (want, S) of the totals) on the moved lattice, or on the lattice in the box (xyz) or
    drifted (tilt)."""
    from tests.virial_util import virial_reference

    box6, mask = LJ_BOXES[box]
    types, _, eps, sig, rcf = _lj_par(par, RC_LIST)
    q, pairs = (_lj_moved(box), _lj_moved_pairs(box)) if moved else (_lj_input(box, box == "tilt"), _lj_pairs(box, box == "tilt"))
    return (lj_reference(q, box6, mask, eps, sig, rcf, types=types, pairs=pairs),
            virial_reference(q, box6, mask, eps, sig, rcf, types=types, pairs=pairs)[:2])


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,par", LJ_CASES)
def test_lj_on_a_held_stream(box, par, full, dtype):
    """The Lennard-Jones forces and totals, scalar and typed: enqueued behind an update behind the delay; then blocking from
    the default stream and from a second side stream behind an asynchronous build on the held stream; then the totals on two
    streams under the caller's fence (fenced_totals)."""
    torch = _torch()
    q1 = _lj_moved(box)
    src, dec = device(q1, dtype), device(rolled(q1), dtype)
    nl = _lj_handle(box, par, full, dtype)
    forces, virial = _lj_calls(nl, par)
    qd = dec.clone()
    fd, wd = _outputs(dtype)
    nl.update(qd, sync=True)
    forces(qd), virial(qd), forces(qd, wait=False, out=fd), virial(qd, wait=False, out=wd)
    torch.cuda.synchronize()
    fd.fill_(-1.0), wd.fill_(-1.0)
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        forces(qd, wait=False, out=fd)
        virial(qd, wait=False, out=wd)
        h.assert_held(f"lj {box} {par} {full} {np.dtype(dtype).name}")
    torch.cuda.synchronize()
    (want, S), (ww, SW) = _lj_refs(box, par, True)
    check_lj(fd.cpu().numpy(), want, S, dtype)
    check_virial(wd.cpu().numpy(), ww, SW, dtype)
    # blocking, from another stream
    q = _lj_input(box, box == "tilt")
    src, dec = device(q, dtype), device(rolled(q), dtype)
    (want, S), (ww, SW) = _lj_refs(box, par, False)
    qd.copy_(dec)
    nl.MakeNeighList(qd)  # (warm: a plain build has buffers that an update's build has not)
    for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
        qd.copy_(dec)
        with held_stream() as h:
            h.copy(qd, src)
            h.assert_held()
            nl.MakeNeighList(qd, sync=False)
            h.assert_held(f"asynchronous build lj {box} {par} {full}")
            with torch.cuda.stream(other):
                f, w = forces(qd), virial(qd)
                other.synchronize()
        check_lj(f.cpu().numpy(), want, S, dtype)
        check_virial(w.cpu().numpy(), ww, SW, dtype)
    # the totals on two streams under the caller's fence: lj_virial and lj_virial_typed are the first users of the scratch
    for w in fenced_totals(nl, virial, qd, src, dec, None, None, f"totals lj {box} {par} {full}"):
        check_virial(w.cpu().numpy(), ww, SW, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,par", LJ_CASES)
def test_histogram_on_a_held_stream(box, par, full, dtype):
    """The pair histogram, untyped (scalar) and typed: enqueued behind an update behind the delay into a zeroed tensor, then
    blocking from the default stream and from a second side stream behind an asynchronous build.  For the untyped histogram of positions alone the decoy
    has the wanted counts (a histogram does not see a relabelling), so there the list is compared with the oracle's as well
    (xyz) -- the typed one counts per pair of types, which stay where they are."""
    torch = _torch()
    box6, mask = LJ_BOXES[box]
    typed = par != "scalar"
    types, rc_ab = _lj_par(par, RC_LIST)[:2]
    q1 = _lj_moved(box)
    ref = hist_r2(lj_pairs(q1, box6, mask, 2.6), N, types, 3 if typed else 1, rc_ab=rc_ab)
    src, dec = device(q1, dtype), device(rolled(q1), dtype)
    nl = _lj_handle(box, par, full, dtype)
    qd = dec.clone()
    nl.update(qd, sync=True)
    hd = nl.pair_histogram(qd, 2.5, 50, typed=typed, wait=False)
    torch.cuda.synchronize()
    hd.zero_()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        nl.pair_histogram(qd, 2.5, 50, typed=typed, wait=False, out=hd)
        h.assert_held(f"histogram {box} {par} {full} {np.dtype(dtype).name}")
    torch.cuda.synchronize()
    check_hist(hd.cpu().numpy(), ref, 2.5, 50, dtype)
    if box == "xyz" and not typed:
        _assert_oracle_list(nl, q1.astype(dtype), box6[:3], mask)
    qd.copy_(dec)
    nl.MakeNeighList(qd)  # (warm: a plain build has buffers that an update's build has not)
    for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
        qd.copy_(dec)
        with held_stream() as h:
            h.copy(qd, src)
            h.assert_held()
            nl.MakeNeighList(qd, sync=False)
            h.assert_held(f"asynchronous build histogram {box} {par} {full}")
            with torch.cuda.stream(other):
                hb = nl.pair_histogram(qd, 2.5, 50, typed=typed)
                other.synchronize()
        check_hist(hb.cpu().numpy(), ref, 2.5, 50, dtype)
        if box == "xyz" and not typed:
            _assert_oracle_list(nl, q1.astype(dtype), box6[:3], mask)


def _assert_oracle_list(nl, q, box, mask, rc=RC_LIST):
    """The handle's list == the oracle's of q at the cut-off rc (open or fully periodic box)."""
    po = _po()
    q = np.ascontiguousarray(q)
    if mask == 0:
        hf = po.build(q, rc, box)
        cnt, kp, lst = (_symmetrised if nl.full_list else _canonical)(hf.key_pointer, hf.sorted_list)
    else:
        assert mask == 7
        hf = (po.build_pbc_full if nl.full_list else po.build_pbc)(q, rc, box)
        cnt, kp, lst = _canonical(hf.key_pointer, hf.sorted_list)
    check_whole(nl, (cnt, kp, lst), ("oracle list", mask, nl.full_list))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box", ["xyz", "tilt"])
def test_pair_vectors_on_a_held_stream(box, full, dtype):
    """nl_pair_vectors_enqueue behind an update behind the delay, with nl_set_pair_images: every image is the float64
    reference's and every vector is pair_vectors_ref's, bit for bit, in the list's own order; the rows beyond the list stay
    untouched.  Then the blocking call from the default stream and from a second side stream.  Half and full, both boxes."""
    from tests.test_pair_images import _entries, image_ref, pair_vectors_ref, same_bits

    torch = _torch()
    box6, mask = LJ_BOXES[box]
    q1 = _lj_moved(box).astype(dtype)
    src, dec = device(q1), device(rolled(q1))
    nl = _handle(box, dtype, full, RC_LIST, images=True)
    nl.set_skin(SKIN)
    nl.Initialize(N)
    qd = dec.clone()
    nl.update(qd, sync=True)
    cap = nl.list_entries() + 4096
    nl.set_capacity(cap)
    nl.update(qd, sync=True)
    out = torch.zeros((cap, 4), dtype=qd.dtype, device="cuda")
    nl.pair_vectors(qd, out=out, wait=False)
    torch.cuda.synchronize()
    out.zero_()
    with held_stream() as h:
        h.copy(qd, src)
        h.assert_held()
        nl.update(qd)
        nl.pair_vectors(qd, out=out, wait=False)
        h.assert_held(f"pair vectors {box} {np.dtype(dtype).name}")
    torch.cuda.synchronize()

    def check(vectors):
        rows, parts, img = _entries(nl)
        assert len(rows) == nl.list_entries() > 50 * N // (1 if full else 2)
        assert not (img != image_ref(q1, box6, mask, rows, parts)[0]).any()
        assert same_bits(vectors[:len(rows)].cpu().numpy(), pair_vectors_ref(q1, box6, dtype, rows, parts, img))
        r2 = vectors[:len(rows), 3].cpu().numpy()
        assert r2.max() <= RC_LIST ** 2 and len(np.unique(rows * N + parts)) == len(rows)
        return len(rows)

    assert not out[check(out):].any()
    if box == "xyz":
        _assert_oracle_list(nl, q1, box6[:3], mask)
    qd.copy_(dec)
    nl.MakeNeighList(qd)  # (warm: a plain build has buffers that an update's build has not)
    for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
        qd.copy_(dec)
        with held_stream() as h:
            h.copy(qd, src)
            h.assert_held()
            nl.MakeNeighList(qd, sync=False)
            h.assert_held(f"asynchronous build pair vectors {box}")
            with torch.cuda.stream(other):
                got = nl.pair_vectors(qd)
                other.synchronize()
        check(got)


# ------------------------------------------------------------------------------------ D: getters, resort, setters
@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("width", [32, 64])
def test_getters_behind_an_asynchronous_build(width, dtype, monkeypatch):
    """Behind an asynchronous build on the held stream, each on a build of its own so that it is the call that waits:
    key_pointer() and key_pointer64() for both build widths (one of them converts, on the build's stream), the transposed
    list against the oracle's full CSR (after a half and a full build), list_checksum(), cell_order() and
    profile_last_build(), before and after which the list is the oracle's."""
    torch = _torch()
    monkeypatch.setenv("NL_OFFSET_WIDTH", str(width))
    key = ("A", 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    n = len(q)
    src, dec = device(q), device(rolled(q))
    qd = dec.clone()
    po = _po()
    for mask, full in ((0, False), (7, True)):
        glob = global_list(key, mask, full)
        fcnt, _, flst = global_list(key, mask, True)
        nl = make_handle(box, n, dtype, mask, full, capacity=int(glob[1][-1]))
        nl.MakeNeighList(qd)  # (warm)

        def build():
            qd.copy_(dec)
            with held_stream() as h:
                h.copy(qd, src)
                h.assert_held()
                nl.MakeNeighList(qd, sync=False)
                h.assert_held(f"getter {width} {dtype} {mask}")

        for bits in (32, 64):
            build()
            kp = nl.full_csr(bits)[0] if full else (nl.key_pointer() if bits == 32 else nl.key_pointer64())
            assert nl.build_info()["offset_bits"] == width
            assert kp.dtype == (torch.int32 if bits == 32 else torch.int64)
            assert np.array_equal(kp.cpu().numpy().astype(np.int64), glob[1]), (bits, width, full)
        build()
        t = nl.neigh_list().cpu().numpy()
        cnt = nl.number_of_partners().cpu().numpy()
        assert np.array_equal(cnt[:n], fcnt)
        assert np.array_equal(np.concatenate([np.sort(t[:cnt[i], i]) for i in range(n)]), flst)
        build()
        assert nl.list_checksum() == (mix_sum(np.arange(n), glob[0], glob[2]), int(glob[1][-1]))
        build()
        order = nl.cell_order().cpu().numpy()
        cells = po.cells(np.ascontiguousarray(q[order]), RC, box)[0]
        assert np.array_equal(np.sort(order), np.arange(n)) and np.all(np.diff(cells) >= 0)
        build()
        check_whole(nl, glob, "before the profile")
        nl.profile_last_build(reps=2)
        check_whole(nl, glob, "after the profile")


def _shifted_pairs(pairs, n):
    """The decoy of an exclusion table: every index moved up by one -- as many pairs, another set."""
    return ((np.asarray(pairs, dtype=np.int64) + 1) % n).astype(np.int32)


@gpu
@pytest.mark.parametrize("pending", [False, True], ids=["built", "pending"])
@pytest.mark.parametrize("tables", ["none", "exclusions", "types"])
def test_resort_behind_the_delay_then_a_rebuild(tables, pending):
    """nl_resort of the positions, the velocities and the ids, all written behind the delay, then a rebuild on the same stream.
    As test_resort_then_rebuild_equals_the_oracle_on_the_permuted_input: the arrays are the inputs permuted by cell_order, and
    the list is the oracle's of the permuted particles; with an exclusion table, and with a type table, which the first
    re-sort after a build relabels: the reference's of the permuted table.
    built: the build whose permutation is applied is synchronised, and a spare array has been re-sorted (which allocates
    nl_resort's buffer and relabels the table, waiting for the device as it does), so the three calls only enqueue: the
    stream is still held behind them and behind the rebuild, and a gather on any stream that runs ahead of the held one
    would permute the decoy.
    pending: the build is asynchronous on the held stream, its positions behind the delay; nl_resort waits for it on the
    host, so this way shows the wait and the results, not the stream of the gather."""
    from tests.test_exclusions import mixed_pairs, remove_pairs
    from tests.test_type_cutoffs import seeded_types, type_filter

    torch = _torch()
    dtype = np.float32
    key = ("B", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["B"]
    n = len(q)
    _, kp0, lst0 = global_list(key, 0, False)
    nl = make_handle(box, n, "float32", capacity=int(kp0[-1]))
    pairs = types = rcm = None
    if tables == "exclusions":
        pairs = mixed_pairs(kp0, lst0, n, 41)
        nl.set_exclusions(pairs, n)
    if tables == "types":
        types, rcm = seeded_types(n, 3, 42, RC)
        nl.set_type_cutoffs(types, rcm)
    rng = np.random.default_rng(43)
    vel = rng.normal(size=(n, 3)).astype(dtype)
    ids = np.arange(n, dtype=np.int32)
    src, dec = device(q), device(rolled(q))
    vsrc, vdec = device(vel), device(rolled(vel))
    isrc, idec = device(ids), device(rolled(ids))
    qd, vd, idd = dec.clone(), vdec.clone(), idec.clone()
    if pending:
        nl.MakeNeighList(qd)  # (warm: every buffer of a build; nl_resort's own buffer is allocated by its first call)
        with held_stream() as h:
            h.copy(qd, src), h.copy(vd, vsrc), h.copy(idd, isrc)
            h.assert_held()
            nl.MakeNeighList(qd, sync=False)
            h.assert_held(f"build before the re-sort {tables}")
            nl.resort(qd, vd, idd)  # (waits for the build: the permutation is its result)
            nl.MakeNeighList(qd, sync=False)
    else:
        qd.copy_(src)
        nl.MakeNeighList(qd)
        spare = torch.arange(n, dtype=torch.int32, device="cuda")
        nl.resort(spare)
        torch.cuda.synchronize()
        qd.copy_(dec)
        with held_stream() as h:
            h.copy(qd, src), h.copy(vd, vsrc), h.copy(idd, isrc)
            h.assert_held()
            nl.resort(qd, vd, idd)
            h.assert_held(f"re-sort {tables}")
            nl.MakeNeighList(qd, sync=False)
            h.assert_held(f"rebuild behind the re-sort {tables}")
        assert torch.equal(idd, spare)
    nl.synchronize()
    order = idd.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n))
    qp = q[order]
    assert np.array_equal(qd.cpu().numpy(), qp) and np.array_equal(vd.cpu().numpy(), vel[order])
    assert np.all(np.diff(_po().cells(np.ascontiguousarray(qp), RC, box)[0]) >= 0)
    want = list_of(qp, box, 0, False)
    if tables == "exclusions":
        inv = np.empty(n, dtype=np.int64)
        inv[order] = np.arange(n)
        want = remove_pairs(want[1], want[2], inv[pairs.astype(np.int64)])
    if tables == "types":
        assert np.array_equal(nl.types().cpu().numpy(), types[order])
        want = type_filter(want[1], want[2], qp, RC, box, 0, dtype, types[order], rcm)
    check_whole(nl, tuple(np.asarray(a, dtype=np.int64) for a in want), ("rebuilt", tables))


@gpu
def test_set_exclusions_takes_pairs_from_the_callers_stream():
    """nl_set_exclusions with a device array written behind the delay on the caller's stream ("may come from any stream"):
    the table is the wanted pairs', not the decoy's, and the build on that stream leaves exactly them out."""
    from tests.test_exclusions import mixed_pairs, remove_pairs, table_csr

    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    n = len(q)
    _, kp0, lst0 = global_list(key, 0, False)
    pairs = mixed_pairs(kp0, lst0, n, 51)
    assert len(table_csr(pairs, n)[1]) == len(table_csr(_shifted_pairs(pairs, n), n)[1])
    psrc, pd = device(pairs), device(_shifted_pairs(pairs, n))
    src, dec = device(q), device(rolled(q))
    qd = dec.clone()
    nl = make_handle(box, n, "float32", capacity=int(kp0[-1]))
    with held_stream() as h:
        h.copy(pd, psrc), h.copy(qd, src)
        h.assert_held()
        nl.set_exclusions(pd, n)
        nl.MakeNeighList(qd, sync=False)
    nl.synchronize()
    off, ids = (t.cpu().numpy() for t in nl.exclusions())
    off_w, ids_w = table_csr(pairs, n)
    assert np.array_equal(off, off_w) and np.array_equal(ids, ids_w)
    check_whole(nl, tuple(np.asarray(a, dtype=np.int64) for a in remove_pairs(kp0, lst0, pairs)), "exclusions")


@gpu
def test_set_type_cutoffs_takes_types_from_the_callers_stream():
    """nl_set_type_cutoffs with a device array written behind the delay on the caller's stream: the handle's copy holds the
    wanted types, and the build on that stream is the reference's of them."""
    from tests.test_type_cutoffs import seeded_types, type_filter

    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    n = len(q)
    _, kp0, lst0 = global_list(key, 0, False)
    types, rcm = seeded_types(n, 3, 61, RC)
    tsrc, td = device(types), device(rolled(types))
    assert not np.array_equal(types, rolled(types))
    src, dec = device(q), device(rolled(q))
    qd = dec.clone()
    nl = make_handle(box, n, "float32", capacity=int(kp0[-1]))
    with held_stream() as h:
        h.copy(td, tsrc), h.copy(qd, src)
        h.assert_held()
        nl.set_type_cutoffs(td, rcm)
        nl.MakeNeighList(qd, sync=False)
    nl.synchronize()
    assert np.array_equal(nl.types().cpu().numpy(), types)
    want = type_filter(kp0, lst0, q, RC, box, 0, np.float32, types, rcm)
    check_whole(nl, tuple(np.asarray(a, dtype=np.int64) for a in want), "types")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_set_charges_reads_the_tensor_in_stream_order(dtype):
    """nl_set_charges keeps a reference: a tensor set while it holds the decoy and written behind the delay is read, by
    the blocking calls of another stream behind an asynchronous build, with the wanted charges."""
    torch = _torch()
    COUL = family("coul")[0]
    box, kind = "xyz", "salt"
    q = _table_input(box, False)
    src, dec = device(q, dtype), device(rolled(q), dtype)
    nl = _family_handle(COUL, box, kind, True, dtype)
    csrc = device(uc.charges(kind), dtype)
    cd = torch.roll(csrc, -1)
    nl.set_charges(cd)
    qd = dec.clone()
    nl.MakeNeighList(qd)
    with held_stream() as h:
        h.copy(qd, src), h.copy(cd, csrc)
        h.assert_held()
        nl.MakeNeighList(qd, sync=False)
        h.assert_held(f"charges {np.dtype(dtype).name}")
        with torch.cuda.stream(torch.cuda.default_stream()):
            f, w = nl.coul_forces(qd), nl.coul_virial(qd)
            torch.cuda.default_stream().synchronize()
    COUL.check(f, w, (), uc.ref(box, False, kind), dtype)


# ------------------------------------------------------------------------------------------ E: slab builds in two parts
def _rolled_within(a, bounds):
    """a with the rows of each segment [bounds[k], bounds[k + 1]) rolled by one among themselves: owned rows stay owned, the
    ghosts of either layer stay in their layer."""
    out = np.array(a)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi - lo > 1:
            out[lo:hi] = np.roll(a[lo:hi], -1, axis=0)
    return out


@gpu
@pytest.mark.parametrize("binning", [None, "1"], ids=["default", "NL_BINNING=1"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_slab_build_in_two_parts_on_a_held_stream(dtype, binning, monkeypatch):
    """Decomposition B1: the owned rows copied behind the delay, nl_make_list_slab_begin, the ghost rows copied, then
    nl_make_list_slab_finish asynchronously; the decoy is the rows rolled within the owned particles and within either ghost
    layer, under the same ids.  Row by row against the oracle (check_rows), half and full, on a warm handle that only
    enqueues."""
    if binning is not None:
        monkeypatch.setenv("NL_BINNING", binning)
    torch = _torch()
    box_name, layers = DECOMPS["B1"]
    key = (box_name, 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES[box_name]
    parts = slab_parts(q, box, RC, layers)
    for full in (False, True):
        glob = global_list(key, 0, full)
        nl = make_handle(box, max(len(p["order"]) for p in parts), dtype, 0, full, capacity=int(glob[1][-1]))
        for part in parts:
            order = part["order"]
            n_own, n_lo = len(part["own"]), len(part["glo"])
            qa = np.array(q[order])
            src, dec = device(qa), device(_rolled_within(qa, (0, n_own, n_own + n_lo, len(order))))
            assert not torch.equal(src[:n_own], dec[:n_own]) and not torch.equal(src[n_own:], dec[n_own:])
            gid = device(order.astype(np.int32))
            qd = dec.clone()
            args = (qd, gid, n_own, n_lo, part["z_lo"], part["z_hi"])
            nl.MakeNeighListSlabBegin(*args)  # (warm, on the decoy)
            nl.MakeNeighListSlabFinish(sync=True)
            with held_stream() as h:
                h.copy(qd[:n_own], src[:n_own])
                h.assert_held()
                nl.MakeNeighListSlabBegin(*args)
                h.copy(qd[n_own:], src[n_own:])
                nl.MakeNeighListSlabFinish(sync=False)
                h.assert_held(f"slab {dtype} {binning} {full} {part['z_lo']}")
            nl.synchronize()
            got = read_slab(nl)
            if binning is not None:
                assert got["stats"]["cap_row"] == 0 and got["info"]["binning"] == "atomic", (got["info"], got["stats"])
            else:
                assert got["info"]["binning"] != "atomic", got["info"]
            check_rows(got, part, glob, (dtype, binning, full))


# ------------------------------------------------------------------------------------- F: two handles, two streams
@gpu
def test_two_handles_on_two_held_streams():
    """Two handles, other inputs (the lattice in the periodic box in fp32, in the open box in fp64), two held streams, the
    enqueues interleaved: update 1, update 2, forces 1, forces 2.  Both lists are the oracle's and both forces are within
    the bound of their float64 reference: the handles share no state."""
    torch = _torch()
    cases = [("xyz", np.float32, False), ("open", np.float64, True)]
    hs, qs = [], []
    for box, dtype, full in cases:
        q = _lj_input(box, False)
        nl = _lj_handle(box, "scalar", full, dtype)
        qd = device(rolled(q), dtype)
        fd = _outputs(dtype)[0]
        nl.update(qd, sync=True)
        nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF, wait=False, out=fd)
        hs.append((nl, qd, fd))
        qs.append(device(q, dtype))
    torch.cuda.synchronize()
    # (stream 1 is held for longer: making stream 2 may pass over up to 7 streams behind whose delay the null stream would
    # wait, 350 ms in all)
    with held_stream(450.0) as h1, held_stream(50.0, settle=False) as h2:
        for h, (nl, qd, fd), src in zip((h1, h2), hs, qs):
            with torch.cuda.stream(h.stream):
                h.copy(qd, src)
                h.assert_held()
                nl.update(qd)
        for h, (nl, qd, fd) in zip((h1, h2), hs):
            with torch.cuda.stream(h.stream):
                nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF, wait=False, out=fd)
        h1.assert_held("two handles, stream 1")
        h2.assert_held("two handles, stream 2")
    torch.cuda.synchronize()
    for (box, dtype, full), (nl, qd, fd) in zip(cases, hs):
        box6, mask = LJ_BOXES[box]
        want, S = lj_reference(_lj_input(box, False), box6, mask, 1.0, 1.0, RCF, pairs=_lj_pairs(box, False))
        check_lj(fd.cpu().numpy(), want, S, dtype)
        _assert_oracle_list(nl, _lj_input(box, False).astype(dtype), box6[:3], mask)

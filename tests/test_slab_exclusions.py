"""Exclusions keyed by global id (nl_set_exclusions_global) on slab, split, whole and distributed builds.

A build with a global table must list exactly the entries (row id a, partner id b) of the plain build with {a, b} not in
the table.  Every expectation comes from the oracle alone: the global list of the undivided box (tests/test_slab_paths.py,
global_list), the excluded pairs removed on the CPU (tests/test_exclusions.py, remove_pairs), cut to the rank's rows
(take_rows); under other ids through `relabelled`.  Every comparison is exact: counts, key_pointer, per-row ascending
partners, nl_number_of_pairs, and nl_list_checksum against mix_sum, whose values add up over the slabs to the checksum of
the global filtered list.  One process builds the slabs of a decomposition one after another; the multi-process cases
(nl_make_list_distributed over gloo) live in tests/slab_excl_worker.py.

The excluded pairs of every case (excluded_pairs) hold, for every slab of the decomposition: owned-owned pairs,
owned-ghost pairs with the smaller id on either side, ghost-ghost pairs; pairs between the top layer and layer 0 (the top
slab's upper ghost: within the cut-off where z is periodic); pairs beyond the cut-off; duplicates and both orders; and a hub
whose row of the table holds more than 32 ids, some of them ghosts of its owner (the binary-search branch of the stage).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from md_neighbor_list_amd import slab
from tests.test_exclusions import remove_pairs, table_csr
from tests.test_periodic_axes import reference as padded_reference
from tests.test_slab_paths import (BOXES, DECOMPS, RC, _canonical, build_slab, check_rows, expected_plan, make_handle, mesh,
                                   mix_sum, read_slab, relabelled, run_decomposition, slab_parts, take_rows)
from tests.test_slab_paths import global_list as paths_global_list
from tests.test_slab_paths import make_input as paths_make_input
from tests.util import ROOT

gpu = pytest.mark.gpu
PER_KIND = 48  # pairs drawn per category and slab


def _torch():
    import torch

    return torch


def _n_max(parts):
    return max(len(p["order"]) for p in parts)


# ------------------------------------------------------------------------------------------------------ inputs


@functools.lru_cache(maxsize=None)
def make_input(box_name, per_cell, dtype_name, kind="uniform", extra=0):
    """The inputs of tests/test_slab_paths.py, and "outside_xy": a tenth of the particles up to 0.9 box lengths outside on
    either side along x and y only (the periodic axes of mask 3; the padded reference of a mixed mask keeps z in the box)."""
    if kind != "outside_xy":
        return paths_make_input(box_name, per_cell, dtype_name, kind, extra)
    q = np.array(paths_make_input(box_name, per_cell, dtype_name, "uniform", 0))
    rng = np.random.default_rng(per_cell + 31)
    k = len(q) // 10
    q[:k, :2] += (rng.choice([-1.0, 1.0], size=(k, 2)) * rng.uniform(0.0, 0.9, size=(k, 2)) * np.array(BOXES[box_name][:2])).astype(q.dtype)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def global_list(key, mask, full):
    """(counts, key_pointer, list) of the undivided box from the oracle alone, as tests/test_slab_paths.py builds it."""
    if key[3] != "outside_xy":
        return paths_global_list(key, mask, full)
    assert mask == 3
    h = padded_reference(make_input(*key), RC, BOXES[key[0]], mask, full=full)
    return _canonical(h.key_pointer, h.sorted_list)


# ------------------------------------------------------------------------------------------------------ the pairs


def excluded_pairs(key, mask, decomp, ids=None, seed=0):
    """[E, 2] particle indices (not ids) with every category of the module docstring present for every slab of `decomp`;
    ids: the id of every particle (default: its index), which decides "the smaller id"."""
    q, box = make_input(*key), BOXES[key[0]]
    n, mz = len(q), mesh(box)[2]
    ids = np.arange(n, dtype=np.int64) if ids is None else ids
    parts = slab_parts(q, box, RC, DECOMPS[decomp][1], mask)
    cnt, kp, lst = global_list(key, mask, True)
    i, j = np.repeat(np.arange(n, dtype=np.int64), cnt), lst
    rng = np.random.default_rng(977 + seed)
    out = []

    def draw(sel, what):
        idx = np.flatnonzero(sel)
        assert len(idx), (key, mask, decomp, what)
        idx = rng.choice(idx, size=min(len(idx), PER_KIND), replace=False)
        out.append(np.stack([i[idx], j[idx]], axis=1))

    for p in parts:
        own, gh = np.zeros(n, bool), np.zeros(n, bool)
        own[p["own"]] = True
        gh[p["glo"]] = gh[p["ghi"]] = True
        draw(own[i] & own[j], "owned-owned")
        draw(own[i] & gh[j] & (ids[i] < ids[j]), "owned-ghost, the owned id smaller")
        draw(own[i] & gh[j] & (ids[i] > ids[j]), "owned-ghost, the ghost id smaller")
        draw(gh[i] & gh[j], "ghost-ghost")
    # across the z wrap: the top slab's upper ghost layer is layer 0
    iz = slab.z_layer(_torch().from_numpy(np.array(q)), box, RC, periodic_z=bool(mask & 4)).numpy()
    top, bot = iz == mz - 1, iz == 0
    if mask & 4:
        draw(top[i] & bot[j], "across the periodic z wrap")
    else:  # (an open box lists no such pair: excluded all the same)
        out.append(np.stack([rng.choice(np.flatnonzero(top), PER_KIND), rng.choice(np.flatnonzero(bot), PER_KIND)], axis=1))
    # the hub: an owned particle of the first slab with the most listed ghost partners; all its partners and 40 strangers
    p = parts[0]
    own, gh = np.zeros(n, bool), np.zeros(n, bool)
    own[p["own"]] = True
    gh[p["glo"]] = gh[p["ghi"]] = True
    ghosts_of = np.bincount(i[own[i] & gh[j]], minlength=n)
    hub = int(np.argmax(ghosts_of))
    assert ghosts_of[hub] > 0
    others = np.setdiff1d(rng.choice(n, size=48, replace=False), [hub])[:40]
    partners = np.union1d(lst[kp[hub]:kp[hub + 1]], others)
    assert len(partners) > 32 and gh[partners].any()
    out.append(np.stack([np.full(len(partners), hub, dtype=np.int64), partners], axis=1))
    # beyond the cut-off (nearly all of them), duplicates, both orders
    far = rng.integers(0, n, size=(PER_KIND, 2))
    out.append(far[far[:, 0] != far[:, 1]])
    pairs = np.concatenate(out)
    quarter = len(pairs) // 4
    pairs = np.concatenate([pairs, pairs[:quarter], pairs[quarter:2 * quarter, ::-1]])
    pairs = pairs[rng.permutation(len(pairs))].astype(np.int64)
    listed = np.isin((pairs[:, 0] << 32) | pairs[:, 1], (i << 32) | j)
    assert listed.any() and not listed.all()  # within the cut-off and beyond it
    return pairs


def filtered(glob, pairs):
    """A canonical global list (rows and partners in particle indices) without the pairs, in the form of global_list."""
    cnt, kp, lst = remove_pairs(glob[1], glob[2], pairs)
    assert cnt.sum() < glob[0].sum()  # (the table does remove something)
    return cnt.astype(np.int64), kp, lst.astype(np.int64)


def set_table(nl, pairs, n_ids, ids=None):
    p = pairs if ids is None else ids[pairs]
    nl.set_exclusions_global(p.astype(np.int64), int(n_ids))


def sparse_ids(n, seed, spread=3):
    """An injective, permuted map of n particles into [0, spread n): most ids name nobody."""
    rng = np.random.default_rng(seed)
    return rng.permutation(spread * n)[:n].astype(np.int64)


# ------------------------------------------------------------------------------------------------------ CPU


def test_union_of_the_ranks_rows_is_the_global_filtered_list():
    """The expectation helper on the 3 x 3 x 7 box: "global filtered list cut to the owned rows", over the ranks of a
    decomposition, is the global filtered list entry for entry, and the numpy checksums of the ranks add up to its
    checksum -- half and full, identity and sparse ids."""
    key = ("A", 8, "float32", "uniform", 0)
    n = len(make_input(*key))
    for decomp in ("A1", "A2"):
        parts = slab_parts(make_input(*key), BOXES["A"], RC, DECOMPS[decomp][1])
        for ids in (None, sparse_ids(n, 5)):
            pairs = excluded_pairs(key, 0, decomp, ids)
            for full in (False, True):
                if ids is None:
                    glob = filtered(global_list(key, 0, full), pairs)
                else:
                    glob = relabelled(filtered(global_list(key, 0, False), pairs), ids, full)
                names = np.arange(n) if ids is None else ids
                seen, total = [], 0
                for p in parts:
                    c, l = take_rows(glob, p["own"])
                    seen.append((np.repeat(names[p["own"]], c) << 32) | l)
                    total = (total + mix_sum(names[p["own"]], c, l)) & (2**64 - 1)
                seen = np.sort(np.concatenate(seen))
                want = np.sort((np.repeat(names, glob[0]) << 32) | glob[2])
                assert np.array_equal(seen, want) and len(np.unique(seen)) == len(seen), (decomp, full)
                assert total == mix_sum(names, glob[0], glob[2]), (decomp, full)
                # no entry of the union is an excluded pair, and only excluded pairs are missing
                a, b = names[pairs[:, 0]], names[pairs[:, 1]]
                ex = np.concatenate([(a << 32) | b, (b << 32) | a])
                assert not np.isin(seen, ex).any()
                if ids is None:
                    plain = global_list(key, 0, full)
                    gone = np.setdiff1d((np.repeat(names, plain[0]) << 32) | plain[2], seen)
                    assert len(gone) and np.isin(gone, ex).all()


def test_the_symbol_is_exported_and_declared():
    from md_neighbor_list_amd import NeighListGPU, _lib

    assert "nl_set_exclusions_global" in _lib.PROTOTYPES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "nl_set_exclusions_global")
    with open(os.path.join(ROOT, "include", "nl_hip.h")) as f:
        assert "int nl_set_exclusions_global(nl_handle_t h, const int32_t* pairs_dev, int64_t n_pairs, int32_t n_ids);" in f.read()
    assert callable(NeighListGPU.set_exclusions_global)


# ------------------------------------------------------------------------------------------------------ GPU, one process


def run_filtered(nl, key, mask, decomp, what, expect=None, **kw):
    """The slabs of `decomp` with the table of excluded_pairs on the handle, half and full, against the oracle."""
    q, box = make_input(*key), BOXES[key[0]]
    parts = slab_parts(q, box, RC, DECOMPS[decomp][1], mask)
    pairs = excluded_pairs(key, mask, decomp)
    set_table(nl, pairs, len(q))
    for full in (False, True):
        nl.set_full_list(full)
        run_decomposition(nl, q, parts, filtered(global_list(key, mask, full), pairs), (what, full), expect, **kw)


@gpu
@pytest.mark.parametrize("decomp", ["A1", "A2", "B2"])
@pytest.mark.parametrize("per_cell,dtype", [(8, "float32"), (30, "float32"), (50, "float32"), (90, "float32"), (30, "float64"),
                                            (90, "float64")])
def test_search_paths(per_cell, dtype, decomp):
    """Case 1: the small instances, one-batch masks, fine rows and dense builds (asserted through build_info), open box."""
    key = (DECOMPS[decomp][0], per_cell, dtype, "uniform", 0)
    parts = slab_parts(make_input(*key), BOXES[key[0]], RC, DECOMPS[decomp][1])
    nl = make_handle(BOXES[key[0]], _n_max(parts), dtype)
    run_filtered(nl, key, 0, decomp, (decomp, per_cell, dtype), dict(expected_plan(per_cell, dtype, 0), offset_bits=32))


@gpu
@pytest.mark.parametrize("decomp", ["A1", "B2"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("mask", [0, 3, 7])
def test_masks_with_particles_outside_the_box(mask, dtype, decomp):
    """Case 2: masks 0, 3 and 7 with a tenth of the particles outside the box (mask 3: outside along its periodic axes x
    and y); under mask 7 the excluded pairs across the z wrap are listed pairs."""
    key = (DECOMPS[decomp][0], 30, dtype, "outside_xy" if mask == 3 else "outside", 0)
    q, box = make_input(*key), BOXES[key[0]]
    assert (q[:, 0] < 0).any() and (q[:, 1] >= box[1]).any() and ((q[:, 2] < 0).any() or mask == 3)
    parts = slab_parts(q, box, RC, DECOMPS[decomp][1], mask)
    nl = make_handle(box, _n_max(parts), dtype, mask)
    run_filtered(nl, key, mask, decomp, (decomp, mask, dtype), dict(masks=True, mask_rows=1, fine_rows=0))


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("form", ["gid4", "w"])
def test_sparse_permuted_ids(form, dtype):
    """Case 3: a gid array and NL_GID_IN_W (int32 bits in F32, int64 bits in F64) with ids scattered over [0, 3 n): the
    table is indexed by id, not by row.  n_ids = 3 n, and 40 n with the gid array: more ids than the handle's own scans
    are sized for (they follow n_max and the mesh)."""
    key = ("A", 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    spread = 40 if form == "gid4" else 3
    ids = sparse_ids(len(q), 21, spread)
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    pairs = excluded_pairs(key, 0, "A1", ids)
    nl = make_handle(box, _n_max(parts), dtype)
    set_table(nl, pairs, spread * len(q), ids)
    off, tab = (t.cpu().numpy() for t in nl.exclusions())  # (either kind, n = n_ids)
    off_w, tab_w = table_csr(ids[pairs], spread * len(q))
    assert np.array_equal(off, off_w) and np.array_equal(tab, tab_w)
    half = filtered(global_list(key, 0, False), pairs)
    for full in (False, True):
        nl.set_full_list(full)
        run_decomposition(nl, q, parts, relabelled(half, ids, full), (form, dtype, full), ids=ids, form=form)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_identity_ids(dtype):
    """Case 3: gid_dev == NULL -- the ids are the slab's own rows (owned, lower ghosts, upper ghosts), the table speaks in
    them, and a table with fewer ids than rows is NL_ERR_ARG at the call."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NLError

    torch = _torch()
    key = ("A", 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    n = len(q)
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    nl = make_handle(box, _n_max(parts), dtype)
    for part in parts:
        order = part["order"]
        ids = np.full(n, -1, dtype=np.int64)
        ids[order] = np.arange(len(order))
        ids[ids < 0] = len(order) + np.arange(n - len(order))
        pairs = excluded_pairs(key, 0, "A1")  # (under a slab's own numbering no ghost has the smaller id)
        here = pairs[(ids[pairs] < len(order)).all(axis=1)]  # (a pair with a particle this slab does not hold names no id of it)
        half = filtered(global_list(key, 0, False), here)
        qa = torch.from_numpy(np.array(q[order])).cuda()
        for full in (False, True):
            nl.set_full_list(full)
            set_table(nl, here, len(order), ids)
            nl.MakeNeighListSlab(qa, None, len(part["own"]), part["z_lo"], part["z_hi"])
            check_rows(read_slab(nl), part, relabelled(half, ids, full), (dtype, part["z_lo"], full), ids=ids)
        few = here[(ids[here] < len(part["own"]) - 1).all(axis=1)]
        assert len(few)
        set_table(nl, few, len(part["own"]) - 1, ids)
        with pytest.raises(NLError) as e:
            nl.MakeNeighListSlab(qa, None, len(part["own"]), part["z_lo"], part["z_hi"])
        assert e.value.code == NL_ERR_ARG


@gpu
@pytest.mark.parametrize("dtype,mask", [("float32", 0), ("float64", 7)])
def test_split_build_equals_the_single_call(dtype, mask):
    """Case 4: nl_make_list_slab_begin + _finish with a table: the oracle's filtered rows, as the single call gives them."""
    key = ("B", 30, dtype, "uniform", 0)
    parts = slab_parts(make_input(*key), BOXES["B"], RC, DECOMPS["B2"][1], mask)
    nl = make_handle(BOXES["B"], _n_max(parts), dtype, mask)
    for split in (True, False):
        run_filtered(nl, key, mask, "B2", (dtype, mask, split), split=split)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_forced_64_bit_offsets(dtype, monkeypatch):
    """Case 5: 64-bit offsets, read through the csr64 getters and through the 32-bit ones."""
    monkeypatch.setenv("NL_OFFSET_WIDTH", "64")
    key = ("A", 30, dtype, "uniform", 0)
    parts = slab_parts(make_input(*key), BOXES["A"], RC, DECOMPS["A1"][1])
    nl = make_handle(BOXES["A"], _n_max(parts), dtype)
    for wide in (True, False):
        run_filtered(nl, key, 0, "A1", (dtype, wide), dict(offset_bits=64), wide=wide)


@gpu
def test_growth_and_capacity_are_counted_before_exclusion():
    """Case 5: a synchronous build that starts from a tiny capacity grows, and its refill is filtered; an asynchronous
    build whose UNFILTERED total exceeds the capacity is NL_ERR_CAPACITY although the filtered list would fit."""
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    part = parts[1]
    for full in (False, True):
        plain = global_list(key, 0, full)
        # enough pairs of the slab's own rows that a capacity fits between the two totals
        c, l = take_rows(plain, part["own"])
        rows = np.repeat(part["own"], c)
        many = np.stack([rows[::3], l[::3]], axis=1)
        pairs = np.concatenate([excluded_pairs(key, 0, "A1"), many])
        glob = filtered(plain, pairs)
        kept, total = int(take_rows(glob, part["own"])[0].sum()), int(c.sum())
        nl = make_handle(box, _n_max(parts), "float32", full=full, capacity=64)
        set_table(nl, pairs, len(q))
        check_rows(build_slab(nl, q, part), part, glob, ("growth", full))
        cap = (kept + total) // 2
        assert kept < cap < total
        nl2 = make_handle(box, _n_max(parts), "float32", full=full, capacity=cap)
        set_table(nl2, pairs, len(q))
        with pytest.raises(NLError) as e:
            build_slab(nl2, q, part, sync=False)
        assert e.value.code == NL_ERR_CAPACITY


@gpu
@pytest.mark.parametrize("form", ["gid4", "w"])
def test_graph_replay_and_a_new_table(form):
    """Case 6: nl_set_graph(1) on slab builds: the second round replays the captured graphs; replacing the table captures
    again and gives the new list."""
    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    pairs = excluded_pairs(key, 0, "A1")
    for full in (False, True):
        plain = global_list(key, 0, full)
        nl = make_handle(box, _n_max(parts), "float32", full=full, graph=True, capacity=plain[1][-1])
        set_table(nl, pairs, len(q))
        keep = {}
        for rnd in (parts, parts[::-1]):
            run_decomposition(nl, q, rnd, filtered(plain, pairs), ("graph", full), sync=False, keep=keep, form=form)
        for _ in range(2):  # the same slab twice: captured, then replayed
            check_rows(build_slab(nl, q, parts[0], sync=False, keep=keep, form=form), parts[0], filtered(plain, pairs), "replay")
        fewer = pairs[: len(pairs) // 2]
        set_table(nl, fewer, len(q))
        for _ in range(2):
            check_rows(build_slab(nl, q, parts[0], sync=False, keep=keep, form=form), parts[0], filtered(plain, fewer), "new table")


@gpu
@pytest.mark.parametrize("dtype,mask", [("float32", 0), ("float64", 7)])
def test_whole_build_equals_the_input_row_table(dtype, mask):
    """Case 7: a whole build with a global table, n == n_ids, gives the CSR and checksum of the same pairs through
    nl_set_exclusions (and the oracle's); n > n_ids is NL_ERR_ARG; nl_resort does not relabel a global table."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NLError

    torch = _torch()
    key = ("B", 30, dtype, "uniform", 0)
    q, box = make_input(*key), BOXES["B"]
    n = len(q)
    pairs = excluded_pairs(key, mask, "B2")
    qd = torch.from_numpy(np.array(q)).cuda()
    for full in (False, True):
        got = []
        for kind in ("rows", "global"):
            nl = make_handle(box, n, dtype, mask, full=full)
            (nl.set_exclusions if kind == "rows" else nl.set_exclusions_global)(pairs, n)
            nl.MakeNeighList(qd, n)
            r = read_slab(nl)
            got.append(r)
            glob = filtered(global_list(key, mask, full), pairs)
            assert np.array_equal(r["counts"], glob[0]) and np.array_equal(r["key_pointer"], glob[1]), (kind, full)
            assert np.array_equal(r["partners"], glob[2]), (kind, full)
            assert r["checksum"] == mix_sum(np.arange(n), glob[0], glob[2]) and r["entries"] == glob[1][-1], (kind, full)
        assert got[0]["checksum"] == got[1]["checksum"] and got[0]["half_pairs"] == got[1]["half_pairs"]
        # (nl is the handle with the global table) the first re-sort after a build relabels an input-row table only
        table = [t.cpu().numpy().copy() for t in nl.exclusions()]
        nl.resort(torch.arange(n, dtype=torch.int32, device="cuda"))
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(table, nl.exclusions()))
        nl.MakeNeighList(qd, n)
        assert read_slab(nl)["checksum"] == got[1]["checksum"]
        small = pairs[(pairs < n - 1).all(axis=1)]
        nl.set_exclusions_global(small, n - 1)
        with pytest.raises(NLError) as e:
            nl.MakeNeighList(qd, n)
        assert e.value.code == NL_ERR_ARG
        nl.MakeNeighList(qd, n - 1)  # (n <= n_ids: fine)


@gpu
def test_errors_and_table_kinds():
    """Case 8: a bad pair is NL_ERR_ARG and keeps the old table; a row id >= n_ids is NL_ERR_ARG from the build, synchronous
    or at the synchronisation of an asynchronous one; the two setters replace each other's table, and only the global kind
    lets a slab build through; clearing returns the plain lists."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    key = ("A", 30, "float32", "uniform", 0)
    q, box = make_input(*key), BOXES["A"]
    n = len(q)
    parts = slab_parts(q, box, RC, DECOMPS["A1"][1])
    part = parts[2]
    pairs = excluded_pairs(key, 0, "A1")
    plain = global_list(key, 0, False)
    glob = filtered(plain, pairs)
    nl = make_handle(box, _n_max(parts), "float32")
    set_table(nl, pairs, n)
    table = [t.cpu().numpy().copy() for t in nl.exclusions()]
    for bad in ([[0, n]], [[-1, 3]], [[5, 5]]):
        with pytest.raises(NLError) as e:
            nl.set_exclusions_global(np.concatenate([pairs[:10], np.array(bad)]), n)
        assert e.value.code == NL_ERR_ARG
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(table, nl.exclusions()))
    check_rows(build_slab(nl, q, part), part, glob, "old table kept")
    # a row whose id the table does not hold: ids up to n - 1, a table of the ids below the largest owned one
    short = int(part["own"].max())
    few = pairs[(pairs < short).all(axis=1)]
    for form in ("gid4", "w"):
        for sync in (True, False):
            set_table(nl, few, short)
            with pytest.raises(NLError) as e:
                build_slab(nl, q, part, form=form, sync=sync)
            assert e.value.code == NL_ERR_ARG, (form, sync)
            set_table(nl, few, n)  # partners beyond the ids of the pairs match nothing: the list without `few`
            check_rows(build_slab(nl, q, part, form=form, sync=sync), part, filtered(plain, few), (form, sync))
    # the kinds
    n_local = len(part["order"])
    local = np.array([[0, 1], [2, 3]])
    nl.set_exclusions(local, n_local)
    with pytest.raises(NLError) as e:
        build_slab(nl, q, part)
    assert e.value.code == NL_ERR_STATE
    set_table(nl, pairs, n)
    check_rows(build_slab(nl, q, part), part, glob, "global replaces rows")
    nl.set_exclusions(local, n_local)
    with pytest.raises(NLError) as e:
        build_slab(nl, q, part)
    assert e.value.code == NL_ERR_STATE
    set_table(nl, pairs, n)
    nl.clear_exclusions()
    with pytest.raises(NLError):
        nl.exclusions()
    for p in parts:
        check_rows(build_slab(nl, q, p), p, plain, "cleared")


# ------------------------------------------------------------------------------------------------------ GPU, several processes


@gpu
@pytest.mark.parametrize("world,case", [
    (2, (30000, (25.0, 25.0, 40.0), 3.3, "float32", 401, False)),   # 12 layers: 6 + 6, half list
    (3, (30000, (25.0, 25.0, 50.0), 3.3, "float64", 402, True)),    # 15 layers: 5 + 5 + 5, full list
])
def test_distributed_build_with_a_global_table(world, case):
    """nl_make_list_distributed with the same global table on every rank, synchronous and asynchronous, twice: between the
    builds every particle moves (owners and ghost counts change) and the table is not set again."""
    from tests.slab_excl_worker import run

    res = run(world, case)
    assert res[0] == "ok"

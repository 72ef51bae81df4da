"""nl_lj_forces, nl_lj_virial and nl_pair_histogram on local-index slab lists (nl_set_local_ids).

A slab build with gid = None stores rows of the caller's buffer, owned rows first and ghosts behind them, and a pair that
crosses a cut is stored by both ranks that see it.  With the switch on the consumers read such a list and each rank computes
its share: the owned rows of the global forces (no reaction to a ghost), the virial totals with a crossing pair weighted 1/2
on either side, and a histogram in which exactly one of the two ranks counts a crossing pair.  The references are the
project's O(N^2) float64 sums over the global box (tests.util, tests.virial_util, tests.hist_util), cut into ranks by
tests.slab_consumer_util; the bounds are those of the whole-box tests: LJ_C u S per force component, VIR_C u S per total,
n_in exactly, the histogram by check_hist; the ranks' counters add up to the whole-box call's bit for bit.

Inputs: the jittered 14^3 lattice (N = 2744, L = 15.75) of lj_lattice(SEED, box, cuts=(2.5, 3.4)) in the boxes open, xy
and xyz, and its drifted variants on the periodic boxes.  List cut-off 3.4 gives 4 z layers, 2.5 gives 6 (DECOMPS).
"""
import functools

import numpy as np
import pytest

from tests.consumer_util import HIST_INPUTS, _handle, _torch
from tests.hist_util import check_hist, hist_count, hist_r2
from tests.slab_consumer_util import local_pairs, rank_forces, rank_hist_r2, rank_split, rank_virial, within
from tests.test_slab_paths import slab_parts
from tests.util import LJ_BOXES, LJ_M, check_lj, lj_drift, lj_lattice, lj_pairs, lj_reference
from tests.virial_util import check_virial, virial_reference

gpu = pytest.mark.gpu
SEED = 11
N = LJ_M ** 3
RCF = 2.5
DTYPES = [np.float32, np.float64]
DECOMPS = {  # name: (list cut-off, [z_lo, z_hi) per rank): the two ghost layers of every slab are distinct, no slab is empty
    "4a": (3.4, ((0, 2), (2, 4))),
    "4b": (3.4, ((0, 1), (1, 3), (3, 4))),
    "6a": (2.5, ((0, 1), (1, 4), (4, 6))),
    "6b": (2.5, tuple((k, k + 1) for k in range(6))),
}
INPUTS = [("open", False), ("xy", False), ("xy", True), ("xyz", False), ("xyz", True)]


def hist_cases(box, rc):
    """(r_max, nbins) per list cut-off: the bins of HIST_INPUTS for the box, r_max 2.5, and 3.0 as well under the list of
    3.4 -- no entry near the list's own cut-off takes part."""
    nbins = HIST_INPUTS[box][1]
    return ((2.5, nbins),) if rc == 2.5 else ((2.5, nbins), (3.0, nbins))


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _input(box, drift):
    """[n, 4] float64 holding float32 values."""
    q = lj_drift(_input(box, False), SEED + 1, box) if drift else lj_lattice(SEED, box, cuts=(2.5, 3.4))
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _pairs(box, drift):
    box6, mask = LJ_BOXES[box]
    return lj_pairs(_input(box, drift), box6, mask, 3.4)


@functools.lru_cache(maxsize=None)
def _parts(box, drift, decomp, dtype):
    """The slabs, filed by the rule of the position type."""
    box6, mask = LJ_BOXES[box]
    rc, layers = DECOMPS[decomp]
    parts = slab_parts(_input(box, drift)[:, :3].astype(dtype), box6[:3], rc, layers, mask)
    assert sorted(np.concatenate([p["own"] for p in parts]).tolist()) == list(range(N)) and all(len(p["own"]) for p in parts)
    return parts


@functools.lru_cache(maxsize=None)
def _global(box, drift, bonds=False):
    """(forces (want, S), virial (want, S), {(r_max, nbins): [r2]}) of the whole box."""
    box6, mask = LJ_BOXES[box]
    q, pairs, ex = _input(box, drift), _pairs(box, drift), (_bonds() if bonds else None)
    w, S, _ = virial_reference(q, box6, mask, 1.0, 1.0, RCF, exclusions=ex, pairs=pairs)
    return lj_reference(q, box6, mask, 1.0, 1.0, RCF, exclusions=ex, pairs=pairs), (w, S), hist_r2(pairs, N, exclusions=ex)


@functools.lru_cache(maxsize=None)
def _expect(box, drift, decomp, dtype, bonds=False, wrong=None):
    """Per slab: dict(f = (want, S), w = (want, S), r2 = [sorted r2 up to 3.4], uncovered).  wrong: one of WRONG."""
    box6, mask = LJ_BOXES[box]
    q, pairs, ex = _input(box, drift), _pairs(box, drift), (_bonds() if bonds else None)
    rc = DECOMPS[decomp][0]
    out = []
    for part in _parts(box, drift, decomp, dtype):
        out.append(dict(
            f=rank_forces(q, box6, mask, RCF, pairs, part, ex, ghost_reaction=wrong == "ghost_reaction"),
            w=rank_virial(N, RCF, pairs, part, ex, ghost_weight=1.0 if wrong == "ghost_weight" else 0.5),
            r2=rank_hist_r2(q, N, 3.4, pairs, part, ex, crossing=wrong if wrong in ("both", "none") else "first"),
            uncovered=rank_split(within(pairs, N, rc), N, part)[2]))
    return out


WRONG = ("ghost_reaction", "ghost_weight", "both", "none")


@functools.lru_cache(maxsize=None)
def _bonds():
    """1-2 bonds along x and along z of the lattice, periodic: the z bonds cross every cut."""
    idx = np.arange(N).reshape(LJ_M, LJ_M, LJ_M)
    return np.concatenate([np.stack([idx.ravel(), np.roll(idx, -1, axis=a).ravel()], axis=1) for a in (0, 2)]).astype(np.int32)


def _rule_holds(box, drift, decomp, dtype, bonds=False, wrong=None):
    """The per-rank expectations against the global reference, through the checkers the GPU tests use."""
    (fw, fS), (w, S), r2 = _global(box, drift, bonds)
    ranks, parts = _expect(box, drift, decomp, dtype, bonds, wrong), _parts(box, drift, decomp, dtype)
    rc = DECOMPS[decomp][0]
    assert not any(r["uncovered"] for r in ranks), "a partner within rc of an owned row is neither owned nor a ghost"
    f = np.zeros((N, 4))
    for r, p in zip(ranks, parts):
        f[p["own"]] = r["f"][0]
    check_lj(f, fw, fS, np.float64)
    if wrong is None:
        assert np.array_equal(f, fw)
    tot = sum(r["w"][0] for r in ranks)
    check_virial(tot, w, S, np.float64)  # (n_in exactly; the 7 sums within float64 summation error)
    assert np.allclose(sum(r["w"][1] for r in ranks), S, rtol=1e-12)
    for r_max, nbins in hist_cases(box, rc):
        got = sum(hist_count(r["r2"], r_max, nbins) for r in ranks)
        check_hist(got, r2, r_max, nbins, dtype)
        assert np.array_equal(got, hist_count(r2, r_max, nbins))


# ------------------------------------------------------------------------------------------------------------ not GPU
@pytest.mark.parametrize("decomp", list(DECOMPS))
@pytest.mark.parametrize("box,drift", INPUTS)
def test_the_rule_adds_up(box, drift, decomp):
    """Per-rank expectations add up to the global reference: histograms and n_in exactly, W and U to float64 summation
    error, the force rows equal the global rows; every partner within rc of an owned row is owned or a ghost."""
    for dtype in DTYPES:
        _rule_holds(box, drift, decomp, dtype)
    parts = _parts(box, drift, decomp, np.float32)
    crossing = sum(len(rank_split(within(_pairs(box, drift), N, RCF), N, p)[1][0]) for p in parts)
    assert crossing > 1000, "the decomposition cuts no pairs"
    # no crossing pair of these inputs has dz == 0: the tie-break of the rule is tested on its own (test_tie_on_dz)
    for p in parts:
        assert (rank_split(within(_pairs(box, drift), N, 3.4), N, p)[1][2][:, 2] != 0).all()


def test_long_rows():
    """At list cut-off 3.4 some half rows and all full rows of the global list exceed 64 entries: the wave's second trip."""
    I, J, _, _ = within(_pairs("xyz", False), N, 3.4)
    assert np.bincount(I, minlength=N).min() > 64
    assert (np.bincount(I[I < J], minlength=N) > 64).sum() > 100


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_rule_is_rejected(wrong):
    """Ghost reactions added, ghost weight 1, crossing pairs counted on both sides or on neither: each fails the checkers."""
    for box, drift, decomp in (("xyz", True, "4b"), ("open", False, "6a")):
        _rule_holds(box, drift, decomp, np.float32)
        with pytest.raises(AssertionError):
            _rule_holds(box, drift, decomp, np.float32, wrong=wrong)


def test_bonds_cross_the_cuts():
    for decomp in ("4b", "6a"):
        for part in _parts("xyz", False, decomp, np.float32):
            own = np.zeros(N, dtype=bool)
            own[part["own"]] = True
            b = _bonds()
            assert (own[b[:, 0]] != own[b[:, 1]]).sum() > 100
            loc = local_pairs(b, part, N)
            assert len(loc) and loc.max() < len(part["order"]) and (loc.max(axis=1) >= len(part["own"])).any()
        _rule_holds("xyz", False, decomp, np.float32, bonds=True)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _tdt(dtype):
    return _torch().float32 if dtype == np.float32 else _torch().float64


def _slab_q(q, part, dtype, stride=4):
    return _torch().from_numpy(np.ascontiguousarray(q[part["order"]][:, :stride].astype(dtype))).cuda()


def _new(box, dtype, full, rc, off=0, local=True, graph=False):
    nl = _handle(box, dtype, full, rc, off)
    if graph:
        nl.set_graph(True)
    if local:
        nl.set_local_ids(True)
    nl.Initialize(N)
    return nl


def _build(nl, qd, part, how="call", sync=True):
    if how == "split":
        nl.MakeNeighListSlabBegin(qd, None, len(part["own"]), len(part["glo"]), part["z_lo"], part["z_hi"])
        nl.MakeNeighListSlabFinish(sync=sync)
    else:
        nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"], sync=sync)


def _consume(nl, qd, box, rc, wait=True):
    """(forces, 8 totals, {(r_max, nbins): counters}) of the last build, on the host."""
    f = nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF, wait=wait)
    w = nl.lj_virial(qd, 1.0, 1.0, rc_force=RCF, wait=wait)
    h = {c: nl.pair_histogram(qd, c[0], c[1], wait=wait) for c in hist_cases(box, rc)}
    _torch().cuda.synchronize()
    return f.cpu().numpy(), w.cpu().numpy(), {c: v.cpu().numpy() for c, v in h.items()}


def _check_rank(got, want, box, rc, dtype, tag):
    f, w, h = got
    print(tag, "n_rows", len(f), "n_in", w[7], "pairs", {c: int(v.sum()) for c, v in h.items()})
    assert f.shape == want["f"][0].shape
    check_lj(f, *want["f"], dtype)
    check_virial(w, *want["w"], dtype)
    for (r_max, nbins), counts in h.items():
        check_hist(counts, want["r2"], r_max, nbins, dtype)


def _walk(nl, box, drift, decomp, dtype, how="call", stride=4, sync=True, bonds=False, wait=True):
    """Every slab of the decomposition on the handle, each checked against its expectation; the ranks' sums."""
    rc = DECOMPS[decomp][0]
    q = _input(box, drift)
    tot_w, tot_h = np.zeros(8), None
    for k, (part, want) in enumerate(zip(_parts(box, drift, decomp, dtype), _expect(box, drift, decomp, dtype, bonds))):
        qd = _slab_q(q, part, dtype, stride)
        if bonds:
            nl.set_exclusions_global(local_pairs(_bonds(), part, N), len(part["order"]))
        _build(nl, qd, part, how, sync)
        if not sync:
            nl.synchronize()
        got = _consume(nl, qd, box, rc, wait)
        _check_rank(got, want, box, rc, dtype, (box, drift, decomp, np.dtype(dtype).name, nl.full_list, k))
        tot_w += got[1]
        tot_h = got[2] if tot_h is None else {c: tot_h[c] + v for c, v in got[2].items()}
    return tot_w, tot_h


@gpu
@pytest.mark.parametrize("decomp", list(DECOMPS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,drift", INPUTS)
def test_matrix(box, drift, full, dtype, decomp):
    """Per slab: forces, virial (n_in exact) and histogram against the rank's reference.  Per decomposition: the ranks' 8
    doubles against the whole-box nl_lj_virial of the same handle, the ranks' counters equal to the whole-box call's."""
    rc = DECOMPS[decomp][0]
    nl = _new(box, dtype, full, rc)
    tot_w, tot_h = _walk(nl, box, drift, decomp, dtype)
    qd = _torch().from_numpy(_input(box, drift).astype(dtype)).cuda()
    nl.MakeNeighList(qd, N)  # (a whole build is unaffected by the switch)
    f, w, h = _consume(nl, qd, box, rc)
    (fw, fS), (ww, wS), r2 = _global(box, drift)
    check_lj(f, fw, fS, dtype)
    check_virial(w, ww, wS, dtype)
    check_virial(tot_w, ww, wS, dtype)
    check_virial(tot_w, w, wS, dtype)
    for c in hist_cases(box, rc):
        check_hist(h[c], r2, c[0], c[1], dtype)
        assert np.array_equal(tot_h[c], h[c]), c


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,decomp", [("xyz", True, "4b"), ("xy", False, "6a"), ("open", False, "4a")])
def test_half_equals_full_per_slab(box, drift, decomp, dtype):
    """Per slab the counters of a half and a full build are equal bit for bit, and the virial of one build is the same 64
    bytes twice."""
    rc = DECOMPS[decomp][0]
    q = _input(box, drift)
    handles = [_new(box, dtype, full, rc) for full in (False, True)]
    for part in _parts(box, drift, decomp, dtype):
        qd = _slab_q(q, part, dtype)
        hists = []
        for nl in handles:
            _build(nl, qd, part)
            a = nl.lj_virial(qd, rc_force=RCF).cpu().numpy()
            b = nl.lj_virial(qd, rc_force=RCF).cpu().numpy()
            assert a.tobytes() == b.tobytes() and a[7] > 0
            hists.append([nl.pair_histogram(qd, *c).cpu().numpy() for c in hist_cases(box, rc)])
        for x, y in zip(*hists):
            assert x.sum() > 1000 and np.array_equal(x, y)


@gpu
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("path", ["off64", "stride3", "split", "graph", "enqueue"])
def test_paths(path, full):
    """64-bit offsets, position stride 3, _begin / _finish, a graph-replayed handle walked over all slabs twice, the
    enqueue variants behind a synchronised build."""
    box, drift, decomp, dtype = "xyz", True, "4b", np.float32
    nl = _new(box, dtype, full, DECOMPS[decomp][0], off=64 if path == "off64" else 0, graph=path == "graph")
    kw = dict(stride3=dict(stride=3), split=dict(how="split"), graph=dict(sync=False), enqueue=dict(wait=False)).get(path, {})
    first = _walk(nl, box, drift, decomp, dtype, **kw)
    if path == "off64":
        assert nl.build_info()["offset_bits"] == 64
    if path == "graph":
        again = _walk(nl, box, drift, decomp, dtype, **kw)  # (replayed; a build does not fix the order of a row's entries,
        check_virial(again[0], first[0], _global(box, drift)[1][1], dtype)  # so two builds agree within the bound)
        assert all(np.array_equal(first[1][c], again[1][c]) for c in first[1])
    (ww, wS) = _global(box, drift)[1]
    check_virial(first[0], ww, wS, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """One graph holds the enqueue variants of all three consumers behind a synchronised slab build; replayed."""
    torch = _torch()
    box, drift, decomp, dtype = "xyz", False, "4b", np.float32
    rc = DECOMPS[decomp][0]
    part, want = _parts(box, drift, decomp, dtype)[1], _expect(box, drift, decomp, dtype)[1]
    nl = _new(box, dtype, full, rc)
    qd = _slab_q(_input(box, drift), part, dtype)
    _build(nl, qd, part)
    r_max, nbins = hist_cases(box, rc)[0]
    fd = torch.empty((len(part["own"]), 4), dtype=torch.float32, device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    hd = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)  # once before the capture: the scratch exists
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nl.lj_forces(qd, rc_force=RCF, wait=False, out=fd)
        nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)
        nl.pair_histogram(qd, r_max, nbins, wait=False, out=hd)
    for k in (1, 2):
        fd.fill_(-1.0), wd.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        check_lj(fd.cpu().numpy(), *want["f"], dtype)
        check_virial(wd.cpu().numpy(), *want["w"], dtype)
        h = hd.cpu().numpy()
        assert (h % k == 0).all()  # (the call adds: two replays, twice the counts)
        check_hist(h // k, want["r2"], r_max, nbins, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("decomp", ["4b", "6a"])
def test_exclusions(decomp, full, dtype):
    """A global table given in the local rows of each slab, with bonds that cross the cuts: the references without them."""
    nl = _new("xyz", dtype, full, DECOMPS[decomp][0])
    tot_w, tot_h = _walk(nl, "xyz", False, decomp, dtype, bonds=True)
    (ww, wS), r2 = _global("xyz", False, True)[1:]
    check_virial(tot_w, ww, wS, dtype)
    qd = _torch().from_numpy(_input("xyz", False).astype(dtype)).cuda()
    nl.set_exclusions_global(_bonds(), N)  # the whole box, the same table in global ids
    nl.MakeNeighList(qd, N)
    for c, counts in tot_h.items():
        check_hist(counts, r2, c[0], c[1], dtype)
        assert np.array_equal(counts, nl.pair_histogram(qd, *c).cpu().numpy())
        with pytest.raises(AssertionError):
            check_hist(counts, _global("xyz", False)[2], c[0], c[1], dtype)
    with pytest.raises(AssertionError):
        check_virial(tot_w, *_global("xyz", False)[1], dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_no_owned_rows(full):
    """n_rows = 0 (a rank that holds ghosts only): the forces are untouched, the totals are 8 zeros, nothing is added."""
    torch = _torch()
    box, decomp, dtype = "xyz", "4b", np.float32
    part = _parts(box, False, decomp, dtype)[1]
    ghosts = dict(part, own=part["own"][:0], order=np.concatenate([part["glo"], part["ghi"]]))
    nl = _new(box, dtype, full, DECOMPS[decomp][0])
    qd = _slab_q(_input(box, False), ghosts, dtype)
    _build(nl, qd, ghosts)
    f = torch.full((4, 4), 7.0, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for name in ("nl_lj_forces", "nl_lj_forces_enqueue"):
        assert getattr(nl._lib, name)(nl._h, qd.data_ptr(), 4, 1.0, 1.0, RCF, f.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (f == 7.0).all()
    for wait in (True, False):
        w = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
        h = torch.full((50,), 7, dtype=torch.int64, device="cuda")
        nl.lj_virial(qd, rc_force=RCF, wait=wait, out=w)
        nl.pair_histogram(qd, 2.5, 50, wait=wait, out=h)
        torch.cuda.synchronize()
        assert (w == 0).all() and (h == 7).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_a_slab_without_ghosts_is_the_whole_build(full, dtype):
    """z_lo = 0 and z_hi = mz under the switch: the results of nl_make_list -- the same counters; forces and totals within
    the bound of each other (two builds do not order a row's entries alike, so their sums differ in the last bits)."""
    torch = _torch()
    box, drift, rc = "xyz", True, 3.4
    qd = torch.from_numpy(_input(box, drift).astype(dtype)).cuda()
    whole, one = _new(box, dtype, full, rc, local=False), _new(box, dtype, full, rc)
    whole.MakeNeighList(qd, N)
    one.MakeNeighListSlab(qd, None, N, 0, one.mesh_size[2])
    a, b = _consume(whole, qd, box, rc), _consume(one, qd, box, rc)
    (fw, fS), (ww, wS), r2 = _global(box, drift)
    check_lj(b[0], fw, fS, dtype)
    check_lj(b[0], a[0].astype(np.float64), fS, dtype)
    check_virial(b[1], ww, wS, dtype)
    check_virial(b[1], a[1], wS, dtype)
    for c in hist_cases(box, rc):
        assert np.array_equal(a[2][c], b[2][c])
        check_hist(b[2][c], r2, c[0], c[1], dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_tie_on_dz(full):
    """A pair across the periodic z face whose folded dz is exactly 0: z_i = 0 and z_j = (float)Lz, which lies below an Lz
    that float32 cannot hold, so the image rule folds with z_j itself.  Both slabs are built; exactly one counts the pair:
    the one that owns the particle with the smaller z as given."""
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    rc, L, Lz = 3.0, 15.75, 15.75 + 2.0 ** -22
    zj = np.float32(Lz)
    assert float(zj) < Lz and np.float32(np.float32(0.0) - zj) + zj == 0
    q = np.array([[1.0, 1.0, 0.0, 0.0], [1.5, 1.0, zj, 0.0]], dtype=np.float32)
    parts = slab_parts(q[:, :3], (L, L, Lz), rc, ((0, 1), (4, 5)), 7)
    assert [p["own"].tolist() for p in parts] == [[0], [1]] and [len(p["order"]) for p in parts] == [2, 2]
    counts, n_in, fx = [], [], []
    for part in parts:
        nl = NeighListGPU(rc, L, L, Lz, dtype=torch.float32, full_list=full, minimum_image=True)
        nl.set_local_ids(True)
        nl.Initialize(2)
        qd = _slab_q(q, part, np.float32)
        _build(nl, qd, part)
        assert nl.list_checksum()[1] == 1  # (the pair is an entry of the owned row on both ranks, half or full)
        counts.append(nl.pair_histogram(qd, 2.5, 5).cpu().numpy())
        n_in.append(float(nl.lj_virial(qd, rc_force=RCF).cpu()[7]))
        fx.append(float(nl.lj_forces(qd, rc_force=RCF).cpu()[0, 0]))
    print(counts, n_in, fx)
    assert counts[0].tolist() == [0, 1, 0, 0, 0] and not counts[1].any()
    assert n_in == [0.5, 0.5]
    assert fx[0] == -fx[1] != 0


@gpu
def test_state_and_arguments():
    torch = _torch()
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError

    box, decomp, dtype = "xyz", "4b", np.float32
    rc = DECOMPS[decomp][0]
    part = _parts(box, False, decomp, dtype)[0]
    q = _input(box, False)
    qd = _slab_q(q, part, dtype)
    gid = torch.from_numpy(part["order"].astype(np.int32)).cuda()
    calls = (lambda nl, wait: nl.lj_forces(qd, rc_force=RCF, wait=wait), lambda nl, wait: nl.lj_virial(qd, rc_force=RCF, wait=wait),
             lambda nl, wait: nl.pair_histogram(qd, 2.5, 50, wait=wait))

    def refused(code, f):
        with pytest.raises(NLError) as e:
            f()
        assert e.value.code == code

    # off (the default): every consumer after a gid = None slab build is NL_ERR_STATE, as before
    nl = _new(box, dtype, False, rc, local=False)
    assert nl.local_ids is False
    _build(nl, qd, part)
    for call in calls:
        for wait in (True, False):
            refused(NL_ERR_STATE, lambda: call(nl, wait))
    # on: no caller ids, no distributed build, no transposed list
    nl.set_local_ids(True)
    assert nl.local_ids is True
    refused(NL_ERR_STATE, nl.key_pointer)  # (the switch changed: the list is gone)
    for ids in (gid, "w"):
        refused(NL_ERR_ARG, lambda: nl.MakeNeighListSlab(qd, ids, len(part["own"]), part["z_lo"], part["z_hi"]))
        refused(NL_ERR_ARG, lambda: nl.MakeNeighListSlabBegin(qd, ids, len(part["own"]), len(part["glo"]), part["z_lo"], part["z_hi"]))
    _build(nl, qd, part)
    kp = nl.key_pointer().cpu().numpy()
    nl.set_local_ids(True)  # the same value: the list stays
    assert np.array_equal(nl.key_pointer().cpu().numpy(), kp)
    refused(NL_ERR_STATE, nl.neigh_list)
    for call in calls:
        for wait in (True, False):
            call(nl, wait)
    with pytest.raises(ValueError):
        nl.rdf(nl.pair_histogram(qd, 2.5, 50), 2.5)
    nl.set_local_ids(False)
    refused(NL_ERR_STATE, nl.key_pointer)
    _build(nl, qd, part)
    for call in calls:
        refused(NL_ERR_STATE, lambda: call(nl, True))
    # a slab build with caller ids made with the switch off stays refused after the switch is set (the list is dropped)
    nl.MakeNeighListSlab(qd, gid, len(part["own"]), part["z_lo"], part["z_hi"])
    nl.set_local_ids(True)
    for call in calls:
        refused(NL_ERR_STATE, lambda: call(nl, True))


@gpu
def test_distributed_build_is_refused():
    """nl_make_list_distributed under the switch is NL_ERR_STATE (its lists hold global ids), before anything is exchanged."""
    import ctypes as C

    torch = _torch()
    from md_neighbor_list_amd import _lib
    from md_neighbor_list_amd._lib import NL_ERR_STATE

    nl = _new("xyz", np.float32, False, 3.4)
    lib = nl._lib
    cb = _lib.SENDRECV_FN(lambda *a: 1)  # (never called: the build is refused first)
    comm = C.c_void_p()
    assert lib.nl_comm_create_callbacks(C.byref(comm), 0, 1, cb, None, torch.cuda.current_device()) == 0
    try:
        qd = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
        assert lib.nl_make_list_distributed(nl._h, comm, qd.data_ptr(), N, 0, None, 1) == NL_ERR_STATE
    finally:
        lib.nl_comm_destroy(comm)


@gpu
def test_failed_list():
    """A slab build has no update, so an enqueue variant called behind a pending asynchronous slab build is NL_ERR_STATE.
    What can run behind one is a graph captured behind an earlier, synchronised build of the same shape: when the
    asynchronous build overflows its capacity the replayed enqueue variants give NaN forces, 8 NaN and add nothing, and
    NL_ERR_CAPACITY comes at nl_synchronize."""
    torch = _torch()
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NL_ERR_STATE, NLError

    box, decomp, dtype = "open", "4a", np.float32
    rc = DECOMPS[decomp][0]
    part, want = _parts(box, False, decomp, dtype)[0], _expect(box, False, decomp, dtype)[0]
    nl = _new(box, dtype, False, rc)
    qd = _slab_q(_input(box, False), part, dtype)
    _build(nl, qd, part)
    nl.set_capacity(nl.half_number_of_pairs() + 64)
    _build(nl, qd, part)
    fd = torch.empty((len(part["own"]), 4), dtype=torch.float32, device="cuda")
    wd = torch.empty(8, dtype=torch.float64, device="cuda")
    hd = torch.zeros(50, dtype=torch.int64, device="cuda")
    nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nl.lj_forces(qd, rc_force=RCF, wait=False, out=fd)
        nl.lj_virial(qd, rc_force=RCF, wait=False, out=wd)
        nl.pair_histogram(qd, 2.5, 50, wait=False, out=hd)
    g.replay()
    torch.cuda.synchronize()
    check_lj(fd.cpu().numpy(), *want["f"], dtype)
    check_virial(wd.cpu().numpy(), *want["w"], dtype)
    before = hd.clone()
    assert int(before.sum()) > 1000
    # the same particles in the same layers, 16 times as dense in x and y: the list no longer fits
    qd[:, :2] *= 0.25
    _build(nl, qd, part, sync=False)
    for wait_free in (lambda: nl.lj_forces(qd, rc_force=RCF, wait=False), lambda: nl.lj_virial(qd, rc_force=RCF, wait=False),
                      lambda: nl.pair_histogram(qd, 2.5, 50, wait=False)):
        with pytest.raises(NLError) as e:
            wait_free()
        assert e.value.code == NL_ERR_STATE
    g.replay()
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    torch.cuda.synchronize()
    assert torch.isnan(fd).all() and torch.isnan(wd).all() and torch.equal(hd, before)

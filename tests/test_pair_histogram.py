"""nl_pair_histogram, nl_pair_histogram_typed and their enqueue variants: the pair-distance histogram of the list against an
O(N^2) float64 count that uses no list (tests.hist_util), and md_neighbor_list_amd.rdf on top of it.

Contract tested (include/nl_hip.h, nl_pair_histogram): integer counts, every stored pair once, half
and full lists the same bytes; a pair falls into bin b iff E_b <= r2 < E_{b+1} with E_k the largest T <= ((k r_max) / nbins)^2.
The checker is a condition, not a tolerance (tests.hist_util check_hist): for every edge the cumulated count lies between
the reference pairs surely below the edge and those plus the pairs within rho of it, rho = 2^-17 (fp32) / 2^-46 (fp64),
relative in r^2.  The designed inputs (HIST_INPUTS: tests.util lj_lattice with every edge among its cuts) have no pair
in any band, in the box and drifted, so there the comparison is equality, bin by bin.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import rdf as R
from tests.hist_util import CAP, band_fraction, check_hist, hist_bands, hist_count, hist_edges2, hist_merge, hist_r2, hist_rho
from tests.consumer_util import BIG_BOX, DTYPES, HIST_INPUTS, N, SEED, _big, _bonds, _handle, _torch
from tests.consumer_util import NBLK_VIRIAL as NBLK
from tests.consumer_util import _lj_input as _input
from tests.consumer_util import _lj_moved as _moved
from tests.util import LJ_BOXES, LJ_L, ROOT, lj_drift, lj_lattice, lj_pairs, lj_type_params

RC = 3.4  # the list cut-off of the designed inputs (rc_ab of lj_type_params(nt, 3.4) too)
MATRIX = [(box, drift) for box in HIST_INPUTS for drift in (False, True) if drift <= (LJ_BOXES[box][1] != 0)]
MAX_BINS, LDS_COUNTERS = 4096, 4096  # include/nl_hip.h (test_header_constants)


def _header(name):
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def _hinput(box, drift=False):
    """[n, 4] float64 holding float32 values: the lattice of `box` with no pair near an edge of HIST_INPUTS[box], 2.5 or 3.4."""
    if drift:
        q = lj_drift(_hinput(box), SEED + 1, box)
    else:
        r_max, nbins = HIST_INPUTS[box]
        cuts = set(np.sqrt(hist_edges2(r_max, nbins)[1:]).tolist()) | {2.5, RC}
        q = lj_lattice(SEED, box, cuts=tuple(sorted(cuts)))
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _hpairs(box, drift=False):
    box6, mask = LJ_BOXES[box]
    return lj_pairs(_hinput(box, drift), box6, mask, 3.6)


@functools.lru_cache(maxsize=None)
def _types(nt, full_table=False):
    """(types, rc_ab) of lj_type_params(nt, 3.4): rc_ab = 3.4 but for the pair (0, nt - 1), which has 0; full_table: 3.4 there too."""
    types, rc = lj_type_params(nt, RC)[:2]
    return types, (np.full_like(rc, RC) if full_table else rc)


@functools.lru_cache(maxsize=None)
def _r2(box, drift=False, nt=0, full_table=False):
    """The reference of an input: sorted r2 per slot (nt = 0: one slot, no types)."""
    if not nt:
        return hist_r2(_hpairs(box, drift), N)
    types, rc = _types(nt, full_table)
    return hist_r2(_hpairs(box, drift), N, types=types, ntypes=nt, rc_ab=rc)


@functools.lru_cache(maxsize=None)
def _lj_r2(box, which, seed=21):
    """References on the lattices of tests.test_lj_consumer (the skin and capture tests): "start" = the shifted lattice,
    "moved" = _moved(box, 0.03, seed)."""
    box6, mask = LJ_BOXES[box]
    q = _input(box, False, True) if which == "start" else _moved(box, 0.03, seed)
    return hist_r2(lj_pairs(q, box6, mask, 2.6), N)


@functools.lru_cache(maxsize=None)
def _big_r2():
    q, _ = _big()
    box6, mask = BIG_BOX
    return hist_r2(lj_pairs(q, box6, mask, 2.6), len(q))


BIG_BINS = 25  # (coarse enough for the cap: test_inputs_meet_the_cap)

EDGE_L, EDGE_SEPS, EDGE_BINS = 63.0, (0.0, 0.5, 1.0, 1.5, 2.5, 2.25), (0, 1, 2, 3, None, 4)


@functools.lru_cache(maxsize=None)
def _edge_dimers():
    """(q[72, 4], want[5]): dimers along each axis, inside the 63-wide box and across a periodic face, at separations that
    are edges of r_max = 2.5 / 5 bins exactly (and one at 2.25); every coordinate is a multiple of 1/8 below 64."""
    q, want = [], np.zeros(5, dtype=np.int64)
    for place in range(2):
        for axis in range(3):
            for k, s in enumerate(EDGE_SEPS):
                p1 = np.zeros(3)
                others = [a for a in range(3) if a != axis]
                p1[others[0]], p1[others[1]] = 5.25 + 10.5 * k, 5.25 + 10.5 * (axis + 3 * place)
                p2 = p1.copy()
                if place == 0:
                    p1[axis], p2[axis] = 21.0, 21.0 + s
                else:
                    p1[axis], p2[axis] = (EDGE_L - 0.5 * s if s else 0.0), 0.5 * s
                q += [p1, p2]
                if EDGE_BINS[k] is not None:
                    want[EDGE_BINS[k]] += 1
    out = np.zeros((len(q), 4))
    out[:, :3] = np.array(q)
    return out, want


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_constants():
    assert _header("NL_HIST_MAX_BINS") == MAX_BINS == 4096
    assert _header("NL_HIST_LDS_COUNTERS") == LDS_COUNTERS >= 1
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    for name in ("nl_pair_histogram", "nl_pair_histogram_enqueue", "nl_pair_histogram_typed", "nl_pair_histogram_typed_enqueue"):
        assert re.search(rf"int {name}\(nl_handle_t h, const void\* q_dev, int32_t q_stride, double r_max, int32_t nbins,\s+"
                         r"uint64_t\* hist_dev,\s+void\* stream\);", text), name
    assert "tests/test_pair_histogram.py" in text


def test_designed_inputs_have_empty_bands():
    """Every designed input, in the box and drifted, typed and not: no reference pair within 2^-17 of an edge, of the
    single bin's edge 2.5 or of the list's cut-off; so the GPU comparison is equality for both dtypes."""
    rho = hist_rho(np.float32)
    for box, drift in MATRIX:
        r_max, nbins = HIST_INPUTS[box]
        q = _hinput(box, drift)
        assert len(q) == N == 2744 and np.array_equal(q[:, :3], q[:, :3].astype(np.float32))
        for rm, nb in ((r_max, nbins), (2.5, 1), (RC, 1)):
            sure, m = hist_bands(_r2(box, drift), rm, nb, rho)
            assert not m.any() and sure[0, -1] > 10000, (box, drift, rm, nb, int(m.sum()))
        if box in ("xyz", "tilt"):
            for nt in (3, 32):
                assert not hist_bands(_r2(box, drift, nt), r_max, nbins, rho)[1].any()


def test_inputs_meet_the_cap():
    """The inputs that cannot be designed stay under the cap of 5 % of their pairs in a band: 4096 bins and the shapes at
    the limit of the LDS counters on the "xyz" lattice, the lattices of the skin tests, the tiled lattice."""
    rho = hist_rho(np.float32)
    frac, total = band_fraction(_r2("xyz"), 2.5, MAX_BINS, rho)
    print("xyz, 4096 bins:", frac, total)
    assert 0.0 < frac <= CAP and total > 50000
    assert band_fraction(_r2("xyz"), 2.5, MAX_BINS, hist_rho(np.float64))[0] == 0.0  # (fp64: exact)
    for nt in (3, 32):
        for nbins in _limit_bins(nt):
            assert band_fraction(_r2("xyz", False, nt), 2.5, nbins, rho)[0] <= CAP
    for box in ("xyz", "tilt"):
        for which in ("start", "moved"):
            assert band_fraction(_lj_r2(box, which), 2.5, 50, rho)[0] <= CAP
    assert band_fraction(_lj_r2("xyz", "moved", 22), 2.5, 50, rho)[0] <= CAP
    assert band_fraction(_big_r2(), 2.5, BIG_BINS, rho)[0] <= CAP


def test_reference_self_checks():
    r_max, nbins = HIST_INPUTS["xyz"]
    one = hist_count(_r2("xyz"), r_max, nbins)
    I, J, d, _ = _hpairs("xyz")
    r2 = (d * d).sum(axis=1)
    assert one.shape == (1, nbins) and one.sum() == ((r2 < r_max * r_max) & (I < J)).sum() > 50000
    for nt in (3, 32):
        types, rc = _types(nt)
        slots = hist_count(_r2("xyz", False, nt), r_max, nbins)
        assert slots.shape == (R.nslots(nt), nbins)
        assert not slots[R.slot(0, nt - 1, nt)].any()  # rc_ab = 0: those pairs are not in the list
        full = hist_count(_r2("xyz", False, nt, True), r_max, nbins)
        assert np.array_equal(full.sum(axis=0), one[0]) and full[R.slot(nt - 1, 0, nt)].any()
        keep = np.arange(R.nslots(nt)) != R.slot(0, nt - 1, nt)
        assert np.array_equal(full[keep], slots[keep])
        # slot / expand_slots round-trip
        seen = sorted(R.slot(a, b, nt) for a in range(nt) for b in range(a, nt))
        assert seen == list(range(R.nslots(nt)))
        big = R.expand_slots(full, nt)
        assert big.shape == (nt, nt, nbins) and np.array_equal(big, big.transpose(1, 0, 2))
        for a in range(nt):
            for b in range(nt):
                assert np.array_equal(big[a, b], full[R.slot(a, b, nt)])
        t = np.asarray(types, dtype=np.int64)
        sel = (I < J) & (r2 < r_max * r_max) & (np.minimum(t[I], t[J]) == 1) & (np.maximum(t[I], t[J]) == 2)
        assert full[R.slot(2, 1, nt)].sum() == sel.sum() > 0
    with pytest.raises(ValueError):
        R.slot(0, 3, 3)
    with pytest.raises(ValueError):
        R.expand_slots(np.zeros((5, 4)), 3)


def test_wrong_results_are_rejected():
    r_max, nbins = HIST_INPUTS["xyz"]
    ref = _r2("xyz", False, 3, True)
    want = hist_count(ref, r_max, nbins)
    check_hist(want, ref, r_max, nbins, np.float32, exact=True)
    check_hist(hist_count(_r2("xyz"), r_max, nbins)[0], _r2("xyz"), r_max, nbins, np.float64, exact=True)
    b = int(np.argmax(want[2, :-1]))
    wrong = {}
    w = want.copy()
    w[2, b] -= 1
    w[2, b + 1] += 1
    wrong["one count moved to the neighbouring bin"] = w
    w = want.copy()
    w[2, b] -= 1
    wrong["one pair dropped"] = w
    w = want.copy()
    w[2, b] += 1
    wrong["one pair doubled"] = w
    wrong["two slots swapped"] = want[[0, 2, 1, 3, 4, 5]]
    wrong["a full list counted twice"] = 2 * want
    for name, w in wrong.items():
        for dtype in DTYPES:
            with pytest.raises(AssertionError):
                check_hist(w, ref, r_max, nbins, dtype)
        assert name
    # in a band the neighbouring bin is allowed, and only there: 4096 bins, a pair within 2^-17 of an edge
    ref1 = _r2("xyz")
    want1 = hist_count(ref1, 2.5, MAX_BINS)[0]
    sure, m = hist_bands(ref1, 2.5, MAX_BINS, hist_rho(np.float32))
    k = int(np.flatnonzero(m[0])[0])
    e2 = hist_edges2(2.5, MAX_BINS)[k]
    below = ref1[0][np.searchsorted(ref1[0], e2 * (1 - hist_rho(np.float32)))] < e2
    w = want1.copy()
    src, dst = (k - 1, k) if below else (k, k - 1)
    assert w[src] > 0
    w[src] -= 1
    w[dst] += 1
    check_hist(w, ref1, 2.5, MAX_BINS, np.float32)
    with pytest.raises(AssertionError):
        check_hist(w, ref1, 2.5, MAX_BINS, np.float64)
    with pytest.raises(AssertionError, match="band"):  # the cap: nobody passes by leaving pairs undecided
        check_hist(want1, [np.repeat(e2, 100)], 2.5, MAX_BINS, np.float32)


def test_rdf():
    """An ideal gas has g = 1 within counting noise; on the lattice the normalisation undoes itself."""
    rng = np.random.default_rng(5)
    q = np.zeros((N, 4))
    q[:, :3] = rng.uniform(0.0, LJ_L, size=(N, 3))
    box6, mask = LJ_BOXES["xyz"]
    hist = hist_count(hist_r2(lj_pairs(q, box6, mask, 2.6), N), 2.5, 25)[0]
    V = LJ_L ** 3
    r_mid, g = R.rdf(hist, 2.5, V, N)
    P = 0.5 * N * (N - 1)
    expected = P * R.shell_volumes(2.5, 25) / V
    assert np.allclose(r_mid, (np.arange(25) + 0.5) * 0.1) and abs(R.shell_volumes(2.5, 25).sum() - 4 * np.pi / 3 * 2.5 ** 3) < 1e-9
    busy = expected >= 100
    assert busy.sum() >= 20
    assert np.all(np.abs(g[busy] - 1.0) <= 5.0 / np.sqrt(expected[busy])), np.abs(g[busy] - 1.0) * np.sqrt(expected[busy])
    r_max, nbins = HIST_INPUTS["xyz"]
    for nt in (0, 3):
        hist = hist_count(_r2("xyz", False, nt, True), r_max, nbins)
        types = np.zeros(N, dtype=np.int64) if not nt else np.asarray(_types(nt)[0], dtype=np.int64)
        cnt = np.bincount(types)
        total = 0.0
        for a in range(max(nt, 1)):
            for b in range(a, max(nt, 1)):
                _, g = R.rdf(hist[R.slot(a, b, max(nt, 1))], r_max, V, cnt[a], None if a == b else cnt[b], frames=1)
                pairs = 0.5 * cnt[a] * (cnt[a] - 1) if a == b else cnt[a] * cnt[b]
                total += (g * pairs * R.shell_volumes(r_max, nbins) / V).sum()
        assert abs(total - hist.sum()) <= 1e-9 * hist.sum()
    assert np.allclose(R.rdf(3 * hist[0], r_max, V, 10, frames=3)[1], R.rdf(hist[0], r_max, V, 10)[1])


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _build(box, dtype, full, q, rc=RC, off=0, stride=4, nt=0, full_table=False, exclusions=None):
    torch = _torch()
    nl = _handle(box, dtype, full, rc, off)
    nl.Initialize(len(q))
    if nt:
        nl.set_type_cutoffs(*_types(nt, full_table))
    if exclusions is not None:
        nl.set_exclusions(exclusions, len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


def _np(t):
    assert t.dtype == _torch().int64 and t.is_cuda and t.is_contiguous()
    return t.cpu().numpy()


def _limit_bins(nt):
    """(the most bins whose nslots x nbins fits the LDS counters, the fewest that do not)"""
    fit = LDS_COUNTERS // R.nslots(nt)
    return fit, fit + 1


# -------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift", MATRIX)
def test_matrix(box, drift, dtype):
    """Every box, mask and position state x dtype x list kind, at the input's designed bins, with one bin, and with r_max
    at the list's cut-off: equal to the reference, and half and full the same bytes.  Offset width and q_stride rotate."""
    r_max, nbins = HIST_INPUTS[box]
    ref = _r2(box, drift)
    k = MATRIX.index((box, drift)) + (dtype == np.float64)
    got = {}
    for full in (False, True):
        nl, qd = _build(box, dtype, full, _hinput(box, drift), off=(32, 64)[(k + full) % 2], stride=(4, 3)[k % 2])
        for rm, nb in ((r_max, nbins), (2.5, 1), (RC, 1), (RC, 16)):
            h = nl.pair_histogram(qd, rm, nb)
            assert h.shape == (nb,)
            h = _np(h)
            check_hist(h, ref, rm, nb, dtype, exact=nb != 16)
            got[full, rm, nb] = h
    for (full, rm, nb), h in got.items():
        assert h.tobytes() == got[False, rm, nb].tobytes() and len(h.tobytes()) == 8 * nb


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_both_counter_paths(full, dtype):
    """Counters in LDS up to NL_HIST_LDS_COUNTERS, straight to the device's tensor beyond: the largest shape that fits and the
    smallest that does not, untyped at 4096 bins (the most; always in LDS), 3 types and 32 (528 slots).  A histogram of
    2 k bins merged in pairs is the one of k bins (the even edges are the same doubles), which compares the two paths."""
    assert LDS_COUNTERS == _header("NL_HIST_LDS_COUNTERS") and MAX_BINS <= LDS_COUNTERS
    q = _hinput("xyz")
    nl, qd = _build("xyz", dtype, full, q)
    h = _np(nl.pair_histogram(qd, 2.5, MAX_BINS))
    check_hist(h, _r2("xyz"), 2.5, MAX_BINS, dtype, exact=True if dtype == np.float64 else None)
    assert h.reshape(-1, 2).sum(axis=1).tobytes() == _np(nl.pair_histogram(qd, 2.5, MAX_BINS // 2)).tobytes()
    for nt in (3, 32):
        nl, qd = _build("xyz", dtype, full, q, nt=nt)
        ref = _r2("xyz", False, nt)
        fit, over = _limit_bins(nt)
        assert R.nslots(nt) * fit <= LDS_COUNTERS < R.nslots(nt) * over and 2 * fit <= MAX_BINS
        in_lds = _np(nl.pair_histogram(qd, 2.5, fit, typed=True))
        check_hist(in_lds, ref, 2.5, fit, dtype)
        check_hist(_np(nl.pair_histogram(qd, 2.5, over, typed=True)), ref, 2.5, over, dtype)
        direct = _np(nl.pair_histogram(qd, 2.5, 2 * fit, typed=True))
        check_hist(direct, ref, 2.5, 2 * fit, dtype)
        assert direct.reshape(R.nslots(nt), fit, 2).sum(axis=2).tobytes() == in_lds.tobytes()
        assert not in_lds[R.slot(0, nt - 1, nt)].any() and in_lds.sum() > 40000


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box", ["xyz", "tilt"])
def test_typed(box, full, dtype):
    """Every slot equals the reference; the (0, nt - 1) slot (rc_ab = 0) stays zero; with every rc_ab set the slots sum to
    the untyped histogram of a handle without a table; one type for everybody gives the untyped bytes."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError

    r_max, nbins = HIST_INPUTS[box]
    q = _hinput(box, True)
    plain, qp = _build(box, dtype, full, q)
    untyped = _np(plain.pair_histogram(qp, r_max, nbins))
    with pytest.raises(NLError) as e:  # no table
        plain.pair_histogram(qp, r_max, nbins, typed=True)
    assert e.value.code == NL_ERR_STATE
    for nt in (3, 32):
        nl, qd = _build(box, dtype, full, q, nt=nt)
        h = nl.pair_histogram(qd, r_max, nbins, typed=True)
        assert h.shape == (R.nslots(nt), nbins)
        h = _np(h)
        check_hist(h, _r2(box, True, nt), r_max, nbins, dtype, exact=True)
        assert not h[R.slot(0, nt - 1, nt)].any() and (h.sum(axis=1) > 0).sum() == R.nslots(nt) - 1
        nl, qd = _build(box, dtype, full, q, nt=nt, full_table=True)
        h = _np(nl.pair_histogram(qd, r_max, nbins, typed=True))
        check_hist(h, _r2(box, True, nt, True), r_max, nbins, dtype, exact=True)
        assert h.sum(axis=0).tobytes() == untyped.tobytes()
        assert _np(nl.pair_histogram(qd, r_max, nbins)).tobytes() == untyped.tobytes()  # (untyped, with a table of 3.4s)
    nl = _handle(box, dtype, full, RC)
    nl.Initialize(N)
    nl.set_type_cutoffs(np.zeros(N, dtype=np.int32), [[RC]])
    nl.MakeNeighList(qp, N)
    h = nl.pair_histogram(qp, r_max, nbins, typed=True)
    assert h.shape == (1, nbins) and _np(h).tobytes() == untyped.tobytes() == _np(nl.pair_histogram(qp, r_max, nbins)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_on_the_edges_exactly(full, dtype):
    """Separations 0, 0.5, 1.0, 1.5, 2.25 and 2.5 with r_max = 2.5 and 5 bins, whose edges and their squares are exact in both
    types: bins 0, 1, 2, 3, 4 and none -- along each axis, in the box and across a periodic face."""
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    q, want = _edge_dimers()
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q) and want.tolist() == [6, 6, 6, 6, 6]
    box6 = (EDGE_L, EDGE_L, EDGE_L, 0.0, 0.0, 0.0)
    assert len(lj_pairs(q, box6, 7, 2.6)[0]) == len(q)  # (ordered pairs) every dimer is a pair, and nothing else is near
    assert np.array_equal(hist_count(hist_r2(lj_pairs(q, box6, 7, 2.6), len(q)), 2.5, 5)[0], want)
    nl = NeighListGPU(2.5, EDGE_L, EDGE_L, EDGE_L, dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=True)
    nl.Initialize(len(q))
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, len(q))
    assert np.array_equal(_np(nl.pair_histogram(qd, 2.5, 5)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_more_rows_than_waves(full, dtype):
    """n = 10976 > 4 x 2048: the grid is capped, waves take a second row, the last turn is ragged."""
    from md_neighbor_list_amd import NeighListGPU

    torch = _torch()
    q, _ = _big()
    n = len(q)
    assert n > 4 * NBLK and n % (4 * NBLK) != 0
    box6, _ = BIG_BOX
    nl = NeighListGPU(2.5, *box6[:3], dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=True)
    nl.Initialize(n)
    qd = torch.from_numpy(q.astype(dtype)).cuda()
    nl.MakeNeighList(qd, n)
    check_hist(_np(nl.pair_histogram(qd, 2.5, BIG_BINS)), _big_r2(), 2.5, BIG_BINS, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_accumulates_and_repeats(full, dtype):
    """The call adds: two calls into one tensor give twice one call, out= is honoured and returned; two fresh calls give
    the same bytes, typed and not, from the enqueue variant too."""
    torch = _torch()
    r_max, nbins = HIST_INPUTS["tilt"]
    for typed in (False, True):
        nl, qd = _build("tilt", dtype, full, _hinput("tilt", True), nt=3 if typed else 0)
        a = nl.pair_histogram(qd, r_max, nbins, typed=typed)
        b = nl.pair_histogram(qd, r_max, nbins, typed=typed, wait=False)
        torch.cuda.synchronize()
        assert _np(a).tobytes() == _np(b).tobytes() and _np(a).sum() > 50000
        out = a.clone()
        assert nl.pair_histogram(qd, r_max, nbins, typed=typed, out=out) is out
        assert np.array_equal(_np(out), 2 * _np(a))
        out.fill_(5)
        nl.pair_histogram(qd, r_max, nbins, typed=typed, out=out)
        assert np.array_equal(_np(out), _np(a) + 5)
        with pytest.raises(TypeError):
            nl.pair_histogram(qd, r_max, nbins, typed=typed, out=torch.zeros(a.shape, dtype=torch.int32, device="cuda"))
        with pytest.raises(TypeError):
            nl.pair_histogram(qd, r_max, nbins + 1, typed=typed, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_nan_position(full, dtype):
    """One particle's x is NaN in the positions of the call (not of the build): its pairs are counted nowhere, everybody
    else's are, and the call returns."""
    torch = _torch()
    r_max, nbins = HIST_INPUTS["xyz"]
    nl, qd = _build("xyz", dtype, full, _hinput("xyz"))
    victim = 1234
    qn = qd.clone()
    qn[victim, 0] = float("nan")
    h = nl.pair_histogram(qn, r_max, nbins)
    torch.cuda.synchronize()
    want = hist_r2(_hpairs("xyz"), N, without=victim)
    assert len(want[0]) < len(_r2("xyz")[0])
    check_hist(_np(h), want, r_max, nbins, dtype, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,off", [("xyz", 32), ("tilt", 64)])
def test_reuse_within_the_skin(box, off, full, dtype):
    """A list kept by nl_update_list, read at moved positions by the enqueue variant: the update is skipped, and the answer
    is that of the current positions, not of the build's."""
    torch = _torch()
    q0, q1 = _input(box, False, True), _moved(box)
    nl = _handle(box, dtype, full, 2.9, off)
    nl.set_skin(0.4)
    nl.Initialize(N)
    qd = torch.from_numpy(q0.astype(dtype)).cuda()
    nl.update(qd, sync=True)
    assert nl.build_info()["offset_bits"] == off
    builds = nl.update_stats()[1]
    first = nl.pair_histogram(qd, 2.5, 50, wait=False)
    qd.copy_(torch.from_numpy(q1.astype(dtype)))
    nl.update(qd)
    h = nl.pair_histogram(qd, 2.5, 50, wait=False)
    torch.cuda.synchronize()
    assert nl.update_stats()[1] == builds
    check_hist(_np(first), _lj_r2(box, "start"), 2.5, 50, dtype)
    check_hist(_np(h), _lj_r2(box, "moved"), 2.5, 50, dtype)
    assert not np.array_equal(_np(h), _np(first))
    if dtype == np.float64:
        with pytest.raises(AssertionError):
            check_hist(_np(h), _lj_r2(box, "start"), 2.5, 50, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_captured(full, dtype):
    """One graph holds the copy of the positions, the update and the histogram into a fixed tensor; replayed at three
    position sets, the tensor holds the sum of the three references.  Nothing is allocated, so a handle's first call may
    be the captured one."""
    torch = _torch()
    sets = [(_input("xyz", False, True), _lj_r2("xyz", "start")), (_moved("xyz"), _lj_r2("xyz", "moved")),
            (_moved("xyz", 0.03, 22), _lj_r2("xyz", "moved", 22))]
    nl = _handle("xyz", dtype, full, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    src = torch.from_numpy(sets[0][0].astype(dtype)).cuda()
    qd = src.clone()
    nl.update(qd, sync=True)
    fresh = _handle("xyz", dtype, full, 2.9)
    fresh.Initialize(N)
    fresh.MakeNeighList(qd, N)
    hd = torch.zeros(50, dtype=torch.int64, device="cuda")
    hf = torch.zeros(50, dtype=torch.int64, device="cuda")
    nl.update(qd)
    nl.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qd.copy_(src)
        nl.update(qd)
        nl.pair_histogram(qd, 2.5, 50, wait=False, out=hd)  # (the first histogram call of either handle)
        fresh.pair_histogram(qd, 2.5, 50, wait=False, out=hf)
    assert not _np(hd).any() and not _np(hf).any()  # captured, not run
    for q, _ in sets:
        src.copy_(torch.from_numpy(q.astype(dtype)))
        g.replay()
    torch.cuda.synchronize()
    total = hist_merge(*(ref for _, ref in sets))
    check_hist(_np(hd), total, 2.5, 50, dtype)
    check_hist(_np(hf), total, 2.5, 50, dtype)  # (its list, of rc = 2.9 at the first set, holds every pair below 2.5 of all three)
    assert _np(hd).sum() > 3 * 50000


@pytest.mark.gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity adds nothing; NL_ERR_CAPACITY comes at
    synchronize; after the synchronous repeat the histogram counts."""
    from md_neighbor_list_amd import NeighListGPU, inputs
    from md_neighbor_list_amd._lib import NL_ERR_CAPACITY, NLError

    torch = _torch()
    q, box = inputs.uniform_box(20000, dtype=np.float32, seed=28, box=(28.0, 28.0, 28.0))
    nl = NeighListGPU(3.3, *box, dtype=torch.float32)
    nl.set_skin(0.4)
    nl.Initialize(len(q))
    nl.set_capacity(1000)
    qd = torch.from_numpy(q).cuda()
    out = torch.full((32,), 7, dtype=torch.int64, device="cuda")
    nl.update(qd)
    nl.pair_histogram(qd, 2.9, 32, wait=False, out=out)
    with pytest.raises(NLError) as e:
        nl.synchronize()
    assert e.value.code == NL_ERR_CAPACITY
    assert (out == 7).all()
    nl.update(qd)  # the host has seen the failure: builds (and fails) again
    with pytest.raises(NLError):
        nl.synchronize()
    nl.update(qd, sync=True)  # grows the list
    h = nl.pair_histogram(qd, 2.9, 32, wait=False)
    torch.cuda.synchronize()
    assert h.sum() > 100000 and (h >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
def test_exclusions(full, dtype):
    """The bonded pairs (every site with its +x neighbour) are absent from the counts."""
    r_max, nbins = HIST_INPUTS["xyz"]
    nl, qd = _build("xyz", dtype, full, _hinput("xyz"), rc=2.5, exclusions=_bonds())
    want = hist_r2(_hpairs("xyz"), N, exclusions=_bonds())
    assert len(want[0]) == len(_r2("xyz")[0]) - len(_bonds())  # every bond is a pair below 3.6
    h = _np(nl.pair_histogram(qd, r_max, nbins))
    check_hist(h, want, r_max, nbins, dtype, exact=True)
    assert h.sum() == hist_count(_r2("xyz"), r_max, nbins).sum() - len(_bonds())
    with pytest.raises(AssertionError):
        check_hist(h, _r2("xyz"), r_max, nbins, dtype)


@pytest.mark.gpu
def test_arguments_and_state():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.4)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    out = torch.zeros(MAX_BINS + 1, dtype=torch.int64, device="cuda")
    d, qp, op = C.c_double, qd.data_ptr(), out.data_ptr()
    calls = [lib.nl_pair_histogram, lib.nl_pair_histogram_enqueue, lib.nl_pair_histogram_typed, lib.nl_pair_histogram_typed_enqueue]
    for f in calls:
        assert f(None, qp, 4, d(2.5), 10, op, None) == NL_ERR_ARG
    assert lib.nl_pair_histogram_enqueue(nl._h, qp, 4, d(2.5), 10, op, None) == NL_ERR_STATE  # no build yet
    nl.MakeNeighList(qd, N)
    for f in calls:
        for nbins in (0, -1, MAX_BINS + 1):
            assert f(nl._h, qp, 4, d(2.5), nbins, op, None) == NL_ERR_ARG
        for r_max in (0.0, -1.0, float("nan"), float("inf")):
            assert f(nl._h, qp, 4, d(r_max), 10, op, None) == NL_ERR_ARG
        assert f(nl._h, None, 4, d(2.5), 10, op, None) == NL_ERR_ARG
        assert f(nl._h, qp, 4, d(2.5), 10, None, None) == NL_ERR_ARG
        for stride in (0, 2, 5):
            assert f(nl._h, qp, stride, d(2.5), 10, op, None) == NL_ERR_ARG
    for f in calls[2:]:  # typed without a table
        assert f(nl._h, qp, 4, d(2.5), 10, op, None) == NL_ERR_STATE
    for bad in (dict(r_max=2.95), dict(r_max=2.6, wait=False)):  # rc = 2.9, skin = 0.4
        with pytest.raises(NLError) as e:
            nl.pair_histogram(qd, nbins=10, **bad)
        assert e.value.code == NL_ERR_ARG, bad
    nl.pair_histogram(qd, 2.9, MAX_BINS)
    nl.pair_histogram(qd, 2.5, 1, wait=False)
    torch.cuda.synchronize()
    assert not out.any()  # nothing refused has written
    with pytest.raises(ValueError):
        nl.pair_histogram(qd[:10], 2.5, 10)
    # a pending plain asynchronous build: the enqueue form refuses, the synchronous one waits
    nl.MakeNeighList(qd, N, sync=False)
    assert lib.nl_pair_histogram_enqueue(nl._h, qp, 4, d(2.5), 10, op, None) == NL_ERR_STATE
    assert lib.nl_pair_histogram(nl._h, qp, 4, d(2.5), 10, op, None) == 0
    torch.cuda.synchronize()
    assert out[:10].sum() > 10000 and not out[10:].any()
    # a table with rc_ab = 0 refuses the untyped call; the typed one looks at the pairs of types that are listed
    types, rc_ab = lj_type_params(3, 2.9)[:2]
    nl.set_type_cutoffs(types, rc_ab)
    nl.MakeNeighList(qd, N)
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            nl.pair_histogram(qd, 2.5, 10, wait=wait)
        assert e.value.code == NL_ERR_ARG
    assert nl.pair_histogram(qd, 2.9, 10, typed=True).shape == (6, 10)
    nl.pair_histogram(qd, 2.5, 10, typed=True, wait=False)
    for bad in (dict(r_max=2.95), dict(r_max=2.6, wait=False)):
        with pytest.raises(NLError) as e:
            nl.pair_histogram(qd, nbins=10, typed=True, **bad)
        assert e.value.code == NL_ERR_ARG, bad
    rc_low = np.where(rc_ab > 0, 2.9, 0.0)
    rc_low[1, 1] = 2.0
    nl.set_type_cutoffs(types, rc_low)
    nl.MakeNeighList(qd, N)
    with pytest.raises(NLError) as e:
        nl.pair_histogram(qd, 2.5, 10, typed=True)  # beyond rc_11
    assert e.value.code == NL_ERR_ARG
    nl.pair_histogram(qd, 2.0, 10, typed=True)
    # a slab build has no histogram
    slab = _handle("open", np.float32, False, 2.9)
    mz = slab.mesh_size[2]
    edge = LJ_L / mz
    inner = q[(q[:, 2] > edge + 0.2) & (q[:, 2] < (mz - 1) * edge - 0.2)]
    slab.Initialize(len(inner))
    qs = torch.from_numpy(inner.astype(np.float32)).cuda()
    slab.MakeNeighListSlab(qs, None, len(inner), 1, mz - 1)
    for wait in (True, False):
        with pytest.raises(NLError) as e:
            slab.pair_histogram(qs, 2.5, 10, wait=wait)
        assert e.value.code == NL_ERR_STATE
    # n == 0 adds nothing
    empty = _handle("open", np.float32, False, 2.9)
    empty.Initialize(16)
    empty.MakeNeighList(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    out.fill_(7)
    assert lib.nl_pair_histogram(empty._h, qp, 4, d(2.5), 10, op, None) == 0
    torch.cuda.synchronize()
    assert (out == 7).all()
    # rdf(): the volume and the counts of the build; periodic boxes only
    with pytest.raises(ValueError):
        nl.rdf(torch.zeros(10, dtype=torch.int64), 2.5)


@pytest.mark.gpu
def test_rdf_of_the_wrapper():
    """NeighListGPU.rdf fills in the box volume and the particle counts: the same g as rdf.rdf given them by hand."""
    r_max, nbins = HIST_INPUTS["tilt"]
    nl, qd = _build("tilt", np.float32, False, _hinput("tilt"), nt=3, full_table=True)
    V = LJ_L ** 3
    h = nl.pair_histogram(qd, r_max, nbins)
    r_mid, g = nl.rdf(h, r_max)
    assert np.array_equal(g, R.rdf(_np(h), r_max, V, N)[1]) and g.max() > 1.0 and not g[:15].any()
    ht = nl.pair_histogram(qd, r_max, nbins, typed=True)
    cnt = np.bincount(_types(3)[0])
    assert np.array_equal(nl.rdf(ht, r_max, types=(2, 0), frames=2)[1], R.rdf(_np(ht)[R.slot(0, 2, 3)], r_max, V, cnt[0], cnt[2], frames=2)[1])
    assert np.array_equal(nl.rdf(ht, r_max, types=(1, 1))[1], R.rdf(_np(ht)[R.slot(1, 1, 3)], r_max, V, cnt[1])[1])
    with pytest.raises(ValueError):
        nl.rdf(ht, r_max)

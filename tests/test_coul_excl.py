"""The excluded-pair term of the charges (nl_set_coul_excl_table, nl_coul_excl_forces, nl_coul_excl_virial and their enqueue
variants) against a float64 loop over the exclusion table's pairs, with an error bound per particle and per component, and the
samplers ewald_excluded and ewald_self of md_neighbor_list_amd.coulomb.

Contract tested (include/nl_hip.h, nl_set_coul_excl_table):
  * |got - want| <= COULX_C u S for every particle and each of fx, fy, fz, pe on its own, and <= COULX_CW u S for each of the 7
    sums of the totals, n_in exactly the distinct excluded pairs: want the float64 sum of tests.util_coul_excl excl_reference,
    S the uncancelled sums with the conditioning of s on the rounding of r2;
  * forces and totals are reproducible bit for bit, and the LDS and the global path compute the same bits;
  * add: the rows are added to the buffer in T; behind nl_coul_forces the buffer holds both terms;
  * nl_coul_forces on the filtered list plus this term is nl_coul_forces on the unfiltered list (one table C for both);
  * a table set by nl_set_exclusions and by nl_set_exclusions_global give the same bits; the relabelled table after nl_resort;
  * a pair outside the table gives NaN to exactly its two particles and to all 8 totals;
  * the state, argument and ordering rules of tests.consumer_contract where they apply.

The constants are not fitted to the kernel.  COULX_C and COULX_CW are 4 x the largest |emulated - want| / (u S) that a numpy
emulation of the rule reaches (tests.util_coul_excl: one rounding per operation, no FMA, every particle's terms in a random
order; the totals with the kernels' own tree in both position types) over util_coul_excl.EMULATED, three orders each;
test_emulation_gives_c recomputes both maxima.  The factor 4 is the margin COUL_C took: the kernel's order is one of many.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from md_neighbor_list_amd import coulomb, pair_table
from tests import consumer_contract as contract
from tests import util_coul_excl as ux
from tests import util_coulomb as uc
from tests.consumer_util import BIG_BOX, CASES, DTYPES, N, R_MAX, R_MIN, _big, _handle, _tdt, _torch
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.consumer_util import _table_pairs as _pairs
from tests.util import LJ_BOXES, LJ_M, ROOT, check_lj, lj_ratio, lj_unit
from tests.util_coul_excl import COULX_C, COULX_CW, EMULATED, EMULATED_MAX, EMULATED_MAX_W, NKX, TOPOLOGIES
from tests.util_coulomb import COUL_C, COUL_CW
from tests.virial_util import check_virial, virial_ratio

GRID = (R_MIN, R_MAX, NKX)
ENTRY = ("nl_coul_excl_forces", "nl_coul_excl_forces_enqueue", "nl_coul_excl_virial", "nl_coul_excl_virial_enqueue")
KINDS = ("salt", "typed3")  # the charge sets of tests.util_coulomb


# --------------------------------------------------------------------------------------------------- CPU: the samplers
def test_symbols():
    """The six entry points are in the header and in the binding."""
    from md_neighbor_list_amd import _lib

    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    for name in ENTRY + ("nl_set_coul_excl_table", "nl_get_coul_excl_table"):
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text), name
    assert int(re.search(r"#define NL_COUL_EXCL_BLOCKS\s+(\d+)", text).group(1)) == 256


def test_ewald_excluded_k_is_the_derivative_of_its_c():
    """K = -C'(r) / r by central differences of the sampler's own C (a table of two knots at r -+ h gives C there)."""
    K, Cv = coulomb.ewald_excluded(0.4, *GRID)
    r = pair_table.knots(*GRID)
    assert K.shape == Cv.shape == (NKX,) and K.dtype == Cv.dtype == np.float64 and np.isfinite(K).all() and (Cv < 0).all()
    h = 1e-5
    for k in range(0, NKX, 29):
        (_, lo), (_, hi) = (coulomb.ewald_excluded(0.4, r[k] + s * h, r[k] + s * h + 1.0, 2) for s in (-1.0, 1.0))
        assert abs(-(hi[0] - lo[0]) / (2 * h) / r[k] - K[k]) <= 1e-8 * (abs(K[k]) + abs(Cv[k]) / r[k] ** 2) + 1e-9, k
    K3, C3 = coulomb.ewald_excluded(0.4, *GRID, prefactor=3.0)
    assert np.array_equal(K3, 3.0 * K) and np.array_equal(C3, 3.0 * Cv)
    assert np.allclose(Cv, [-math.erf(0.4 * v) / v for v in r], rtol=1e-15, atol=0)


def test_sampler_identities():
    """ewald_real.C - ewald_excluded.C = prefactor / r (erfc + erf = 1), the same for K with 1 / r^3; ewald_self against a hand
    sum."""
    r = pair_table.knots(*GRID)
    Kr, Cr = coulomb.ewald_real(0.4, *GRID, prefactor=2.5)
    Kx, Cx = coulomb.ewald_excluded(0.4, *GRID, prefactor=2.5)
    assert np.allclose(Cr - Cx, 2.5 / r, rtol=1e-14, atol=0) and np.allclose(Kr - Kx, 2.5 / r ** 3, rtol=1e-13, atol=0)
    q = [1.0, -2.0, 0.5]
    assert coulomb.ewald_self(0.4, q, prefactor=3.0) == pytest.approx(-3.0 * 0.4 / math.sqrt(math.pi) * (1.0 + 4.0 + 0.25), rel=1e-15)
    assert coulomb.ewald_self(0.4, np.zeros(5)) == 0.0 and isinstance(coulomb.ewald_self(0.4, q), float)
    assert "excluded" in coulomb.__doc__ and "ewald_self" in coulomb.__doc__


# --------------------------------------------------------------------------------------------------- CPU: the checker
def test_topologies():
    """Row lengths of both topologies, and every pair inside (0.85, 2.5) on every input: the longest is the 1-3 pair, <= 2.47."""
    for box, drift in CASES:
        box6, mask = LJ_BOXES[box]
        for topo in TOPOLOGIES:
            given, unique = ux.topology(topo, box)
            lo, hi = ux.assert_in_range(_input(box, drift), box6, mask, unique)
            assert 0.92 < lo and hi < 2.47
            off, ids = ux.csr(unique, N)
            rows = np.diff(off)
            assert off[-1] == 2 * len(unique) == len(ids)
            if topo == "chains":
                assert set(rows.tolist()) == ({4} if mask & 1 else {2, 3, 4})
                assert len(given) > len(unique) and (given[:, 0] > given[:, 1]).any() and (given[:, 0] < given[:, 1]).any()
            else:
                idx = np.arange(N).reshape(LJ_M, LJ_M, LJ_M)
                assert rows[idx[ux.HUB]] == 26 and rows[idx[ux.EIGHT]] == 8 and rows[idx[ux.NINE]] == 9
                assert (rows == 0).sum() > N // 5 and (rows == 0).reshape(LJ_M, -1)[:, 3].all() and N % 32 != 0
                assert sorted(set(rows.tolist())) == [0, 1] + ([4, 5] if mask & 1 else [2, 3, 4, 5]) + [8, 9, 26]
    _, unique = ux.topology("chains", "open")
    assert len(unique) < len(ux.topology("chains", "xyz")[1])  # cut at the face


def test_reference_is_the_gradient_of_its_energy():
    """excl_reference's forces against the central difference of its own total energy, tilted and periodic, random charges, a
    potential linear in r^2 (C = c (r_max^2 - r^2): the table interpolates it exactly), on a chain that crosses the faces."""
    rng = np.random.default_rng(3)
    m_, a = 5, 1.125
    box6, mask = (m_ * a, m_ * a, m_ * a, a, -a, 2 * a), 7
    idx = np.arange(m_ ** 3).reshape(m_, m_, m_)
    g = np.stack(np.meshgrid(*(np.arange(m_),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (g + 0.5) * a + rng.uniform(-0.1, 0.1, size=g.shape)
    p = ux._chain_pairs(idx, True)
    unique = np.unique(np.stack([p.min(axis=1), p.max(axis=1)], axis=1), axis=0)
    r_max, h = 2.6, 1e-5
    K, Cv = pair_table.sample(lambda r: 0.9 * (r_max ** 2 - r * r), lambda r: -1.8 * r, 0.4, r_max, 33)
    chg = rng.uniform(-1.0, 1.0, size=len(q))
    (want, S), (w, SW) = ux.excl_reference(q, box6, mask, K, Cv, 0.4, r_max, chg, unique)
    for i in (0, 7, idx[4, 2, 2], idx[0, 0, 4]):
        for c in range(3):
            e = []
            for sgn in (1.0, -1.0):
                pp = q.copy()
                pp[i, c] += sgn * h
                e.append(ux.excl_reference(pp, box6, mask, K, Cv, 0.4, r_max, chg, unique)[0][0][:, 3].sum())
            fd = -(e[0] - e[1]) / (2 * h)
            assert abs(fd - want[i, c]) <= 1e-6 * S[i, c], (i, c, fd, want[i, c])
    assert np.abs(want[:, :3].sum(axis=0)).max() <= 1e-12 * S[:, :3].sum()  # Newton's third law in the reference
    assert abs(w[6] - want[:, 3].sum()) <= 1e-12 * SW[6] and w[7] == len(unique)


def _emulated(box, drift, topo, kind, T, defect=None):
    box6, mask = LJ_BOXES[box]
    I, J = ux.ordered(ux.topology(topo, box)[1])
    return I, ux.excl_emulate_pairs(_input(box, drift), box6, mask, *ux.excl_tab(), R_MIN, R_MAX, uc.charges(kind), T, I, J, defect)


def test_emulation_gives_c():
    """COULX_C and COULX_CW = 4 x the largest |emulated - want| / (u S) of a numpy emulation of the kernel's arithmetic (never
    the kernel) against the float64 reference: per particle and component in fp32, the totals in both position types."""
    worst, worst_w = np.zeros(4), np.zeros(7)
    assert len(EMULATED) == 9 and {e[2] for e in EMULATED} == set(TOPOLOGIES)
    for box, drift, topo, kind in EMULATED:
        (want, S), (ww, SW) = ux.ref(box, drift, topo, kind)
        vals = {T: _emulated(box, drift, topo, kind, T) for T in DTYPES}
        for order in range(3):
            rng = np.random.default_rng(100 + order)
            I, v32 = vals[np.float32]
            r = lj_ratio(ux.excl_emulate(N, I, v32, rng), want, S, np.float32).max(axis=0)
            rw = []
            for T in DTYPES:
                w = ux.excl_virial_emulate(N, I, vals[T][1], rng)
                assert w[7] == ww[7]
                rw.append(virial_ratio(w, ww, SW, T))
            print(box, drift, topo, kind, order, r.round(2), rw[0].round(3), rw[1].round(3))
            worst, worst_w = np.maximum(worst, r), np.maximum(worst_w, np.maximum(*rw))
    print("largest ratio per column", worst, worst_w)
    assert worst.max() <= EMULATED_MAX <= COULX_C / 4
    assert worst_w.max() <= EMULATED_MAX_W <= COULX_CW / 4
    assert EMULATED_MAX - worst.max() < 0.01 and EMULATED_MAX_W - worst_w.max() < 0.001  # the constants are the measured maxima
    assert COULX_C == 4 * EMULATED_MAX and COULX_CW == 4 * EMULATED_MAX_W


def test_bound_is_sharp():
    """COULX_C u S stays below a quarter of what the weakest single pair at r_max gives a component (|q| >= 0.5)."""
    Fm, Um = ux.weakest(*ux.excl_tab(), R_MAX, uc.Q_MIN)
    u = lj_unit(np.float32)
    for box, drift in CASES:
        for topo in TOPOLOGIES:
            (_, S), _ = ux.ref(box, drift, topo, "typed3")
            assert np.all(COULX_C * u * S[:, :3].max(axis=1) <= 0.25 * Fm) and np.all(COULX_C * u * S[:, 3] <= 0.25 * Um)


def test_wrong_results_are_rejected():
    """The checkers under the fp32 bounds refuse every mistake of util_coul_excl.DEFECTS made in the emulator: q_j for q_i q_j,
    C and K swapped, an entry counted with weight 1 in the totals, the term left out of pe, the plain difference instead of
    the nearest image on a chain that crosses a face.  The emulator without a defect passes."""
    for box, drift, topo, kind in (("xyz", False, "chains", "typed3"), ("tilt", True, "mixed", "typed3")):
        (want, S), (ww, SW) = ux.ref(box, drift, topo, kind)
        rng = np.random.default_rng(5)
        I, vals = _emulated(box, drift, topo, kind, np.float32)
        check_lj(ux.excl_emulate(N, I, vals, rng), want, S, np.float32, c=COULX_C)
        check_virial(ux.excl_virial_emulate(N, I, vals, rng), ww, SW, np.float32, c=COULX_CW)
        for defect in ux.DEFECTS:
            I, vals = _emulated(box, drift, topo, kind, np.float32, defect)
            with pytest.raises(AssertionError):
                if defect == "an entry with weight 1 in the totals":
                    check_virial(ux.excl_virial_emulate(N, I, vals, rng, defect), ww, SW, np.float32, c=COULX_CW)
                else:
                    check_lj(ux.excl_emulate(N, I, vals, rng, defect), want, S, np.float32, c=COULX_C)


# ------------------------------------------------------------------------------------------------------ GPU helpers
class _WithCharges:
    """The library as tests.consumer_contract calls it -- fn(handle, q, stride, out, stream) -- with the charge pointer (and
    add = 0 for the forces) put in for the four entry points; every other call, and a call that brings its own charge pointer,
    goes through unchanged."""

    def __init__(self, lib, charges):
        self.__dict__.update(_lib=lib, _charges=charges)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY:
            return fn
        mid = (0,) if "forces" in name else ()  # (add)
        return lambda *a: fn(*a) if len(a) > 5 else fn(*a[:3], self._charges.data_ptr(), a[3], *mid, a[4])


def _charge_tensor(nl, values):
    return _torch().from_numpy(np.array(values, dtype=np.float64)).to(nl.dtype).cuda()


def _set(nl, kind, rc=None, nkx=NKX):
    """kind = "topology/box[/global]": the topology's exclusions (by row, or keyed by id with n_ids = N), the excluded-pair
    table and the rock-salt charges onto an initialised handle."""
    topo, box = kind.split("/")[:2]
    given = ux.topology(topo, box)[0]
    (nl.set_exclusions_global if kind.endswith("/global") else nl.set_exclusions)(given, N)
    nl.set_excluded_coulomb_table(*ux.excl_tab(nkx), R_MIN, R_MAX)
    nl.set_charges(_charge_tensor(nl, uc.charges("salt")))
    if not isinstance(nl._lib, _WithCharges):  # (tests.consumer_contract calls the entry points through nl._lib)
        nl._lib = _WithCharges(nl._lib, nl._charges)


def _check(f, w, refs, dtype, rows=None):
    (want, S), (ww, SW) = refs
    f, w = f.cpu().numpy(), w.cpu().numpy()
    print(np.dtype(dtype).name, lj_ratio(f, want, S, dtype).max(axis=0).round(2), virial_ratio(w, ww, SW, dtype).round(2))
    check_lj(f, want, S, dtype, c=COULX_C, rows=rows)
    if rows is None:
        check_virial(w, ww, SW, dtype, c=COULX_CW)
        assert abs(w[6] - f[:, 3].astype(np.float64).sum()) <= (COULX_C + COULX_CW) * lj_unit(dtype) * SW[6]
    return f, w


def _kind_ref(box, drift, kind):
    return ux.ref(box, drift, kind.split("/")[0], "salt")


def _consumer(kinds):
    return contract.Consumer(
        forces="coul_excl_forces", virial="coul_excl_virial", scratch="coul_excl_virial", clear="clear_excluded_coulomb_table",
        info="excluded_coulomb_table_info", entry=ENTRY, set=_set, kinds=kinds, ref=_kind_ref,
        moved_ref=lambda box, kind: ux.moved_ref(box, kind.split("/")[0], "salt"), extra=lambda nl: (),
        check=lambda f, w, x, refs, dtype, rows=None: _check(f, w, refs, dtype, rows), half_lists=True, local_slabs=False)


COULX = _consumer(("chains/xyz", "mixed/xyz"))
gpu = pytest.mark.gpu


def _built(q, box, dtype, topo, kind="salt", full=False, rc=2.9, stride=4, global_table=False, given=None, n=None):
    """(handle, device positions) after one whole build with the topology's exclusions, the table and the charges set."""
    torch = _torch()
    n = len(q) if n is None else n
    nl = _handle(box, dtype, full, rc)
    nl.Initialize(len(q))
    given = ux.topology(topo, box)[0] if given is None else given
    (nl.set_exclusions_global if global_table else nl.set_exclusions)(given, n)
    nl.set_excluded_coulomb_table(*ux.excl_tab(), R_MIN, R_MAX)
    nl.set_charges(_charge_tensor(nl, uc.charges(kind) if len(q) == N else np.resize(uc.charges(kind), len(q))))
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, len(q))
    return nl, qd


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_matrix(case, dtype, monkeypatch):
    """Every box, mask and position state x both topologies x both dtypes; q_stride, the charge set, the list kind and LDS
    against global rotate through the cases.  n_in is exactly the distinct pairs; forces and totals twice for the same bytes."""
    box, drift = CASES[case]
    q = _input(box, drift)
    for p, topo in enumerate(TOPOLOGIES):
        k = case + p + (dtype == np.float64)
        stride, kind, lds, full = (4, 3)[k % 2], KINDS[(k // 2) % 2], (k // 3) % 2 == 0, (k // 2 + p) % 2 == 1
        monkeypatch.setenv("NL_TABLE_LDS", "1" if lds else "0")
        nl, qd = _built(q, box, dtype, topo, kind, full=full, stride=stride)
        assert qd.shape[1] == stride and nl.excluded_coulomb_table_info() == dict(nknots=NKX, r_min=R_MIN, r_max=R_MAX, lds=lds)
        f, w = nl.coul_excl_forces(qd), nl.coul_excl_virial(qd)
        assert f.shape == (N, 4) and f.dtype == _tdt(dtype) and w.shape == (8,) and w.dtype == _torch().float64
        refs = ux.ref(box, drift, topo, kind)
        f, w = _check(f, w, refs, dtype)
        assert w[7] == len(ux.topology(topo, box)[1]) == refs[1][0][7]
        assert f.tobytes() == nl.coul_excl_forces(qd).cpu().numpy().tobytes()
        assert w.tobytes() == nl.coul_excl_virial(qd).cpu().numpy().tobytes() and len(w.tobytes()) == 64


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_lds_and_global_paths(dtype, monkeypatch):
    """A table set under NL_TABLE_LDS=0 is read from global memory; on one list both paths give the same bits, forces and
    totals, both topologies.  A table beyond NL_TABLE_LDS_BYTES takes the global path by itself."""
    text = open(os.path.join(ROOT, "include", "nl_hip.h")).read()
    lds_bytes = int(re.search(r"#define NL_TABLE_LDS_BYTES\s+(\d+)", text).group(1))
    knot = 4 * np.dtype(dtype).itemsize
    box, drift = "tilt", True
    for topo in TOPOLOGIES:
        monkeypatch.delenv("NL_TABLE_LDS", raising=False)
        nl, qd = _built(_input(box, drift), box, dtype, topo)
        assert nl.excluded_coulomb_table_info()["lds"] and NKX * knot <= lds_bytes
        lds = _check(nl.coul_excl_forces(qd), nl.coul_excl_virial(qd), ux.ref(box, drift, topo), dtype)
        monkeypatch.setenv("NL_TABLE_LDS", "0")
        nl.set_excluded_coulomb_table(*ux.excl_tab(), R_MIN, R_MAX)
        assert not nl.excluded_coulomb_table_info()["lds"]
        glo = nl.coul_excl_forces(qd).cpu().numpy(), nl.coul_excl_virial(qd).cpu().numpy()
        assert lds[0].tobytes() == glo[0].tobytes() and lds[1].tobytes() == glo[1].tobytes()
    monkeypatch.delenv("NL_TABLE_LDS", raising=False)
    nkx = 4096
    if nkx * knot > lds_bytes:  # (fp64: 128 KiB)
        nl.set_excluded_coulomb_table(*ux.excl_tab(nkx), R_MIN, R_MAX)
        assert nl.excluded_coulomb_table_info() == dict(nknots=nkx, r_min=R_MIN, r_max=R_MAX, lds=False)
        box6, mask = LJ_BOXES[box]
        refs = ux.excl_reference(_input(box, drift), box6, mask, *ux.excl_tab(nkx), R_MIN, R_MAX, uc.charges("salt"), ux.topology("mixed", box)[1])
        _check(nl.coul_excl_forces(qd), nl.coul_excl_virial(qd), refs, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("topo", TOPOLOGIES)
def test_add(topo, dtype):
    """add=True into a buffer of known values equals add=False plus those values, computed in T, empty rows included; and
    behind coul_forces the buffer holds the two results added in T."""
    torch = _torch()
    box, drift = "xyz", True
    nl, qd = _built(_input(box, drift), box, dtype, topo, full=True)
    f = nl.coul_excl_forces(qd)
    known = torch.from_numpy(np.random.default_rng(9).uniform(-3.0, 3.0, size=(N, 4))).to(_tdt(dtype)).cuda()
    buf = known.clone()
    assert nl.coul_excl_forces(qd, out=buf, add=True) is buf
    assert torch.equal(buf, known + f) and not torch.equal(buf, known)
    with pytest.raises(ValueError):
        nl.coul_excl_forces(qd, add=True)
    F = np.zeros(64)
    nl.set_pair_table(F, F, R_MIN, R_MAX)
    nl.set_coulomb_table(*uc.coul_tab(), R_MIN, R_MAX)
    fl = nl.coul_forces(qd)
    both = nl.coul_excl_forces(qd, wait=False, out=fl.clone(), add=True)
    assert torch.equal(both, fl + f) and torch.isfinite(both).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box,drift,topo", [("xyz", False, "chains"), ("tilt", True, "mixed"), ("open", False, "chains")])
def test_filtered_list_plus_this_term_is_the_unfiltered_list(box, drift, topo, dtype):
    """A pair table of zeros and one charge table C on (0.85, 2.5) for both terms: coul_forces on the list built with the
    exclusions plus coul_excl_forces equals coul_forces on the list built without them, and so do U and W.  Three results are
    compared, each within its own bound of its float64 reference, and the references agree exactly in exact arithmetic:
    the match is within COUL_C u S_filtered + COULX_C u S_excluded on the one side plus COUL_C u S_unfiltered on the other
    (totals: the same with the CW constants).  The sum of the two terms is taken in float64 on the host: no third rounding."""
    torch = _torch()
    box6, mask = LJ_BOXES[box]
    q = _input(box, drift)
    K, Cv = uc.coul_tab()
    zero = np.zeros(64)
    m = uc.Model(zero, zero, R_MIN, R_MAX, K, Cv, R_MIN, R_MAX, uc.charges("salt"))
    unique = ux.topology(topo, box)[1]
    I, J, d, raw = _pairs(box, drift)
    keys = np.concatenate([unique[:, 0] * N + unique[:, 1], unique[:, 1] * N + unique[:, 0]])
    keep = ~np.isin(I * N + J, keys)
    assert (~keep).sum() == 2 * len(unique)  # every excluded pair is within the list's reach
    (_, S_all), (_, SW_all) = uc.coul_reference(q, box6, mask, m, (I, J, d, raw))
    (_, S_fil), (_, SW_fil) = uc.coul_reference(q, box6, mask, m, (I[keep], J[keep], d[keep], raw[keep]))
    (_, S_ex), (ww_ex, SW_ex) = ux.excl_reference(q, box6, mask, K, Cv, R_MIN, R_MAX, uc.charges("salt"), unique)
    got = {}
    for excl in (False, True):
        nl = _handle(box, dtype, True, 2.9)
        nl.Initialize(N)
        if excl:
            nl.set_exclusions(ux.topology(topo, box)[0], N)
            nl.set_excluded_coulomb_table(K, Cv, R_MIN, R_MAX)
        nl.set_pair_table(zero, zero, R_MIN, R_MAX)
        nl.set_coulomb_table(K, Cv, R_MIN, R_MAX)
        nl.set_charges(_charge_tensor(nl, uc.charges("salt")))
        qd = torch.from_numpy(q.astype(dtype)).cuda()
        nl.MakeNeighList(qd, N)
        f, w = nl.coul_forces(qd).cpu().numpy().astype(np.float64), nl.coul_virial(qd).cpu().numpy()
        if excl:
            f, w = f + nl.coul_excl_forces(qd).cpu().numpy(), w + nl.coul_excl_virial(qd).cpu().numpy()
        got[excl] = f, w
    u = lj_unit(dtype)
    assert np.abs(got[False][0]).max() > 0.1 and got[True][1][7] == got[False][1][7] and ww_ex[7] == len(unique)
    assert np.all(np.abs(got[True][0] - got[False][0]) <= u * (COUL_C * (S_fil + S_all) + COULX_C * S_ex))
    assert np.all(np.abs(got[True][1][:7] - got[False][1][:7]) <= u * (COUL_CW * (SW_fil + SW_all) + COULX_CW * SW_ex))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_table_source(dtype):
    """A table set by nl_set_exclusions and the same pairs set by nl_set_exclusions_global with n_ids == n give the same bits;
    n_ids > n is NL_ERR_ARG from all four calls."""
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NLError

    box, drift, topo = "hex", True, "mixed"
    out = []
    for glob in (False, True):
        nl, qd = _built(_input(box, drift), box, dtype, topo, global_table=glob)
        off, ids = (t.cpu().numpy() for t in nl.exclusions())
        want_off, want_ids = ux.csr(ux.topology(topo, box)[1], N)
        assert np.array_equal(off, want_off) and np.array_equal(ids, want_ids)
        out.append((nl.coul_excl_forces(qd).cpu().numpy().tobytes(), nl.coul_excl_virial(qd).cpu().numpy().tobytes()))
    assert out[0] == out[1]
    nl, qd = _built(_input(box, drift), box, dtype, topo, global_table=True, n=N + 5)
    for call in (nl.coul_excl_forces, nl.coul_excl_virial):
        for wait in (True, False):
            with pytest.raises(NLError) as e:
                call(qd, wait=wait)
            assert e.value.code == NL_ERR_ARG


@gpu
@pytest.mark.parametrize("topo", TOPOLOGIES)
def test_after_resort(topo):
    """Positions and charges permuted by nl_resort, a rebuild: the relabelled table gives the permuted forces and the totals of
    the box."""
    box, drift, kind, dtype = "xyz", True, "typed3", np.float32
    nl, qd = _built(_input(box, drift), box, dtype, topo, kind)
    order = nl.cell_order().cpu().numpy().copy()
    assert not np.array_equal(order, np.arange(N)) and np.array_equal(np.sort(order), np.arange(N))
    chg = nl._charges
    nl.resort(qd, chg)
    assert np.array_equal(chg.cpu().numpy(), uc.charges(kind)[order].astype(dtype))
    nl.MakeNeighList(qd, N)
    inv = np.empty(N, dtype=np.int64)
    inv[order] = np.arange(N)
    u = inv[ux.topology(topo, box)[1]]
    want_off, want_ids = ux.csr(np.unique(np.stack([u.min(axis=1), u.max(axis=1)], axis=1), axis=0), N)
    off, ids = (t.cpu().numpy() for t in nl.exclusions())
    assert np.array_equal(off, want_off) and np.array_equal(ids, want_ids)
    (want, S), (ww, SW) = ux.ref(box, drift, topo, kind)
    _check(nl.coul_excl_forces(qd), nl.coul_excl_virial(qd), ((want[order], S[order]), (ww, SW)), dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["beyond r_max", "coincident"])
def test_a_pair_outside_the_table(what, dtype):
    """One pair beyond r_max (a bond across the open box: the wrapped bond of the periodic chains, which the open box does not
    fold) or one coincident pair: NaN in exactly its two particles and in all 8 totals, nowhere else."""
    box = "open" if what == "beyond r_max" else "xyz"
    box6, mask = LJ_BOXES[box]
    q = _input(box, False).copy()
    idx = np.arange(N).reshape(LJ_M, LJ_M, LJ_M)
    if what == "beyond r_max":
        a, b = int(idx[0, 5, 6]), int(idx[LJ_M - 1, 5, 6])
    else:
        a, b = int(idx[6, 7, 5]), int(idx[7, 7, 5])
        q[b, :3] = q[a, :3]
    given = np.concatenate([ux.topology("chains", box)[0], [[a, b]]]).astype(np.int32)
    unique = np.unique(np.stack([given.min(axis=1), given.max(axis=1)], axis=1).astype(np.int64), axis=0)
    if what == "coincident":  # b moved onto a: its 1-3 partner at x + 2 is now 3.4 away, take that bond out
        drop = {(min(b, int(idx[9, 7, 5])), max(b, int(idx[9, 7, 5])))}
        unique = np.array([p for p in unique.tolist() if tuple(p) not in drop])
        given = unique.astype(np.int32)
    refs = ux.excl_reference(q, box6, mask, *ux.excl_tab(), R_MIN, R_MAX, uc.charges("salt"), unique)
    nans = np.isnan(refs[0][0]).any(axis=1)
    assert np.array_equal(np.flatnonzero(nans), sorted((a, b))) and np.isnan(refs[1][0]).all()
    nl, qd = _built(q, box, dtype, "chains", given=given)
    f, w = nl.coul_excl_forces(qd).cpu().numpy(), nl.coul_excl_virial(qd).cpu().numpy()
    assert np.isnan(w).all() and w.shape == (8,)
    assert np.array_equal(np.isnan(f), np.repeat(nans[:, None], 4, axis=1))
    check_lj(f, *refs[0], dtype, c=COULX_C, rows=~nans)


@gpu
def test_the_grid():
    """10976 rows are 343 blocks' worth of 32 for at most NL_COUL_EXCL_BLOCKS = 256 blocks: the second trip is ragged, 87 of the
    256 blocks take it and the others leave the loop.  Every row against the reference, the totals twice for the same bytes."""
    q, _ = _big()
    box6, mask = BIG_BOX
    unique = ux.big_chains()
    assert len(q) == 10976 == 343 * 32 and 256 < 343 < 2 * 256 and len(unique) == 2 * len(q)
    ux.assert_in_range(q, box6, mask, unique)
    chg = np.resize(uc.charges("typed3"), len(q))
    refs = ux.excl_reference(q, box6, mask, *ux.excl_tab(), R_MIN, R_MAX, chg, unique)
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    nl = NeighListGPU(2.9, *box6[:3], dtype=torch.float32, minimum_image=True)
    nl.Initialize(len(q))
    nl.set_exclusions(unique.astype(np.int32), len(q))
    nl.set_excluded_coulomb_table(*ux.excl_tab(), R_MIN, R_MAX)
    nl.set_charges(_charge_tensor(nl, chg))
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    nl.MakeNeighList(qd, len(q))
    f, w = _check(nl.coul_excl_forces(qd), nl.coul_excl_virial(qd), refs, np.float32)
    assert w[7] == len(unique) and w.tobytes() == nl.coul_excl_virial(qd).cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------ the contract
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("box,topo", [("xyz", "chains"), ("tilt", "mixed")])
def test_reuse_within_the_skin(box, topo, full, dtype):
    contract.reuse_within_the_skin(COULX, box, f"{topo}/{box}", full, dtype)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_captured(full):
    """One graph holds the copy of the positions, the update, the forces and the totals; replayed at two position sets.  The
    charges are read, not copied: changed in place they change the next replay, and so does a table of the same size."""
    def before(nl, qd, fd, wd):
        nl.coul_excl_virial(qd, wait=False, out=wd)  # once before the capture: the scratch exists
        nl.synchronize()

    def after(nl, replay):
        box6, mask = LJ_BOXES["xyz"]
        K, Cv = coulomb.ewald_excluded(0.7, R_MIN, R_MAX, NKX, prefactor=3.0)
        nl.set_excluded_coulomb_table(K, Cv, R_MIN, R_MAX)
        chg = -0.5 * uc.charges("salt")
        chg[::3] *= 2.0
        nl._charges.copy_(_charge_tensor(nl, chg))
        _check(*replay(), ux.excl_reference(_moved("xyz")[0], box6, mask, K, Cv, R_MIN, R_MAX, chg, ux.topology("chains", "xyz")[1]), np.float32)

    contract.captured(COULX, full, before, after)


@gpu
def test_failed_list():
    """An enqueue behind an asynchronous build that overflowed its capacity: NaN rows and 8 NaN totals, NL_ERR_CAPACITY at
    synchronize; after the synchronous repeat both are finite.  The bonds join particles 2 i and 2 i + 1 of a uniform random
    box of edge 28, anywhere up to 28 sqrt(3) = 48.5 apart: the table runs from 1e-3 to 49."""
    def set_tables(nl):
        n = 20000
        nl.set_exclusions(np.arange(n, dtype=np.int32).reshape(-1, 2), n)
        nl.set_excluded_coulomb_table(*coulomb.ewald_excluded(uc.ALPHA, 1e-3, 49.0, NKX), 1e-3, 49.0)
        nl.set_charges(_charge_tensor(nl, np.where(np.arange(n) % 2 == 0, 1.0, -1.0)))

    contract.failed_list(COULX, set_tables, lambda nl, qd: None)


@gpu
@pytest.mark.parametrize("full", [False, True])
def test_distributed_lists_are_refused(full):
    """(A global table: a table by rows refuses the distributed build itself.)"""
    contract.distributed_lists_are_refused(_consumer(("chains/xyz/global",)), full)


@gpu
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("full", [False, True])
def test_slab_lists_are_refused(full, local):
    """A slab build, with and without nl_set_local_ids, filtered by a global table: NL_ERR_STATE from all four calls (with
    local ids the pair table's calls take the list)."""
    from md_neighbor_list_amd._lib import NL_ERR_STATE, NLError
    from tests.consumer_util import _tab
    from tests.test_slab_paths import slab_parts

    torch = _torch()
    box, dtype, rc = "xyz", np.float32, 3.4
    box6, mask = LJ_BOXES[box]
    q = _input(box, False)
    part = slab_parts(q[:, :3].astype(dtype), box6[:3], rc, ((0, 2), (2, 4)), mask)[0]
    nl = _handle(box, dtype, full, rc)
    nl.set_local_ids(local)
    nl.Initialize(N)
    _set(nl, "chains/xyz/global")
    nl.set_charges(_charge_tensor(nl, uc.charges("salt")[part["order"]]))
    F, U, _, _ = _tab("morse")
    nl.set_pair_table(F, U, R_MIN, R_MAX)
    qd = torch.from_numpy(np.ascontiguousarray(q[part["order"]].astype(dtype))).cuda()
    nl.MakeNeighListSlab(qd, None, len(part["own"]), part["z_lo"], part["z_hi"])
    if local:
        assert torch.isfinite(nl.table_forces(qd)).all()
    for call in (nl.coul_excl_forces, nl.coul_excl_virial):
        for wait in (True, False):
            with pytest.raises(NLError) as e:
                call(qd, wait=wait)
            assert e.value.code == NL_ERR_STATE


@gpu
def test_state_and_arguments():
    from md_neighbor_list_amd._lib import NL_ERR_ARG, NL_ERR_STATE, NLError, load

    torch = _torch()
    lib = load()
    K, Cv = ux.excl_tab()
    given = ux.topology("chains", "open")[0]
    q = _input("open", False)
    nl = _handle("open", np.float32, False, 2.9)
    nl.set_skin(0.3)
    nl.Initialize(N)
    qd = torch.from_numpy(q.astype(np.float32)).cuda()
    cd = _charge_tensor(nl, uc.charges("salt"))
    fd = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    shim = _WithCharges(lib, cd)
    calls = contract.entry_calls(COULX, shim, fd, out)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    set_tab = lambda: nl.set_excluded_coulomb_table(K, Cv, R_MIN, R_MAX)  # noqa: E731
    info = dict(nknots=NKX, r_min=R_MIN, r_max=R_MAX, lds=True)
    # neither table, then each alone: NL_ERR_STATE
    assert nl.excluded_coulomb_table_info() is None and lib.nl_get_coul_excl_table(nl._h, None, None, None, None) == NL_ERR_STATE
    nl.MakeNeighList(qd, N)
    for tables in ((), (set_tab,), (nl.clear_excluded_coulomb_table, lambda: nl.set_exclusions(given, N), lambda: nl.MakeNeighList(qd, N))):
        for t in tables:
            t()
        for fn, o in calls:
            assert fn(nl._h, qd.data_ptr(), 4, o.data_ptr(), None) == NL_ERR_STATE
    set_tab()
    assert nl.excluded_coulomb_table_info() == info  # (no pair table needed, for the getter or for the calls)
    # no charges: NULL is NL_ERR_ARG, through the wrapper too
    assert lib.nl_coul_excl_forces(nl._h, qd.data_ptr(), 4, None, fd.data_ptr(), 0, None) == NL_ERR_ARG
    assert lib.nl_coul_excl_forces_enqueue(nl._h, qd.data_ptr(), 4, None, fd.data_ptr(), 1, None) == NL_ERR_ARG
    assert lib.nl_coul_excl_virial(nl._h, qd.data_ptr(), 4, None, out.data_ptr(), None) == NL_ERR_ARG
    assert lib.nl_coul_excl_virial_enqueue(nl._h, qd.data_ptr(), 4, None, out.data_ptr(), None) == NL_ERR_ARG
    for call in (nl.coul_excl_forces, nl.coul_excl_virial):
        with pytest.raises(NLError) as e:
            call(qd)
        assert e.value.code == NL_ERR_ARG
        with pytest.raises(TypeError):
            call(qd, charges=cd.double())
        with pytest.raises(ValueError):
            call(qd, charges=cd[:-1].contiguous())
    nl.set_charges(cd)
    want = nl.coul_excl_virial(qd).cpu().numpy()
    refs = ux.ref("open", False, "chains")
    _check(nl.coul_excl_forces(qd), nl.coul_excl_virial(qd, charges=cd.clone()), refs, np.float32)
    # the setter's arguments: each refused, and the table that was set is kept
    bad_k, bad_c = K.copy(), Cv.copy()
    bad_k[7], bad_c[-1] = np.inf, np.nan
    big = np.zeros(4097)
    for args in ((NKX, R_MIN, R_MAX, dp(K), None), (NKX, R_MIN, R_MAX, None, dp(Cv)), (1, R_MIN, R_MAX, dp(K), dp(Cv)),
                 (-3, R_MIN, R_MAX, dp(K), dp(Cv)), (4097, R_MIN, R_MAX, dp(big), dp(big)), (NKX, 0.0, R_MAX, dp(K), dp(Cv)),
                 (NKX, -1.0, R_MAX, dp(K), dp(Cv)), (NKX, R_MAX, R_MAX, dp(K), dp(Cv)), (NKX, R_MIN, np.inf, dp(K), dp(Cv)),
                 (NKX, np.nan, R_MAX, dp(K), dp(Cv)), (NKX, R_MIN, R_MAX, dp(bad_k), dp(Cv)), (NKX, R_MIN, R_MAX, dp(K), dp(bad_c))):
        assert lib.nl_set_coul_excl_table(nl._h, *args) == NL_ERR_ARG, args[:3]
        assert nl.excluded_coulomb_table_info() == info
    assert lib.nl_set_coul_excl_table(None, NKX, R_MIN, R_MAX, dp(K), dp(Cv)) == NL_ERR_ARG
    assert lib.nl_get_coul_excl_table(None, None, None, None, None) == NL_ERR_ARG
    assert nl.coul_excl_virial(qd).cpu().numpy().tobytes() == want.tobytes() and np.isfinite(want).all()
    with pytest.raises(TypeError):
        nl.set_excluded_coulomb_table(K, Cv[:-1], R_MIN, R_MAX)
    with pytest.raises(TypeError):
        nl.set_excluded_coulomb_table(np.zeros((2, 8)), np.zeros((2, 8)), R_MIN, R_MAX)
    contract.call_arguments(calls, nl, qd)
    contract.setter_keeps_the_list(nl, qd, set_tab)
    # no reach: a list shorter than the table (rc = 2.9 - skin 0.3 against r_max 2.7) is no obstacle, wait or enqueue
    nl.set_excluded_coulomb_table(*ux.excl_tab(NKX, R_MIN, 2.7), R_MIN, 2.7)
    for wait in (True, False):
        assert torch.isfinite(nl.coul_excl_forces(qd, wait=wait)).all() and torch.isfinite(nl.coul_excl_virial(qd, wait=wait)).all()
    set_tab()
    contract.clearing(COULX, nl, qd, set_tab, lambda: lib.nl_set_coul_excl_table(nl._h, 0, R_MIN, R_MAX, dp(K), dp(Cv)))
    set_tab()
    # a first call of the totals inside a capture, on a handle whose scratch does not exist yet
    fresh = _handle("open", np.float32, False, 2.9)
    fresh.Initialize(N)
    _set(fresh, "chains/open")
    fresh.MakeNeighList(qd, N)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(NLError) as e:
            fresh.coul_excl_virial(qd, wait=False)
        fresh.coul_excl_forces(qd, wait=False, out=fd)
    assert e.value.code == NL_ERR_STATE

    def set_empty(empty):  # (a table by rows would refuse the build of no rows: keyed by id, 16 ids)
        empty.set_exclusions_global(np.array([[0, 1]], dtype=np.int32), 16)
        empty.set_excluded_coulomb_table(K, Cv, R_MIN, R_MAX)

    contract.no_particles(COULX, shim, False, set_empty, qd, fd, out)

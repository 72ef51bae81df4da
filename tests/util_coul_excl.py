"""What tests/test_coul_excl.py checks the excluded-pair term against (nl_set_coul_excl_table, nl_coul_excl_forces,
nl_coul_excl_virial): the bonded topologies, a float64 loop over the exclusion table's pairs at their
nearest image, a numpy emulation of the kernel's arithmetic in the position type, and the constants of the bound
|got - want| <= c u S (check_lj, check_virial) with the S defined here.

Inputs: the table family's of tests.consumer_util and tests.util_coulomb -- the 2744-particle lattice, the boxes and position
states of CASES, the "salt" and random ("typed3") charge sets, the grid (R_MIN, R_MAX) = (0.85, 2.5).  The table is Ewald's
C = -PREFACTOR erf(ALPHA r) / r with NKX knots: a grid of its own.

Topologies, the smallest shapes at which the 8-lane walk can go wrong (every pair inside (0.85, 2.5): assert_in_range):
  * "chains": 1-2 and 1-3 pairs along x of every lattice row, periodic where x is, cut at the face of the open box: rows of 2
              to 4 ids; given in both orders and with duplicates;
  * "mixed":  chains on three quarters of the lattice rows, the others unbonded (empty rows, whole groups idle); one site bonded
              to all 26 sites of its 3 x 3 x 3 neighbourhood (4 trips of its group, the last ragged), one row of exactly 8 ids
              and one of 9; n = 2744 is no multiple of 32, so the last block is ragged.
"""
import functools

import numpy as np

from md_neighbor_list_amd import coulomb, pair_table
from tests.consumer_util import N, R_MAX, R_MIN
from tests.consumer_util import _table_input as _input
from tests.consumer_util import _table_moved as _moved
from tests.util import LJ_BOXES, LJ_M, emulate_pairs, lj_list_separations
from tests.util_coulomb import ALPHA, PREFACTOR, charges
from tests.util_table import _block_sum, _sum_rows, table_device_form
from tests.virial_util import _AB

# 4 x the largest |emulated - want| / (u S) of test_coul_excl.test_emulation_gives_c: per particle and column in fp32, and the 7
# totals in both position types.  The measured maxima stand beside them; the kernel is never consulted.
EMULATED_MAX, EMULATED_MAX_W = 1.44, 0.355  # measured: 1.4336 per particle (fz; pe 1.089) and 0.3543 for the totals (W_yy)
COULX_C = 5.76
COULX_CW = 1.42

TOPOLOGIES = ("chains", "mixed")
NKX = 384
HUB, EIGHT, NINE = (6, 4, 3), (3, 8, 3), (10, 8, 7)  # lattice sites of the rows of 26, 8 and 9 ids ("mixed"), all interior
# what the emulation that fixes COULX_C and COULX_CW runs over: nine inputs, both topologies, both charge sets
EMULATED = [("open", False, "chains", "salt"), ("xyz", False, "mixed", "typed3"), ("xyz", True, "chains", "typed3"),
            ("tilt", False, "mixed", "salt"), ("tilt", True, "chains", "salt"), ("xy", True, "mixed", "typed3"),
            ("hex", True, "chains", "typed3"), ("hex", False, "mixed", "salt"), ("xy", False, "chains", "salt")]
DEFECTS = ("qj for qq", "C and K swapped", "an entry with weight 1 in the totals", "no term in pe", "the plain difference")


# ------------------------------------------------------------------------------------------------------- topologies
def _idx():
    return np.arange(N).reshape(LJ_M, LJ_M, LJ_M)  # [x][y][z], as tests.util lj_lattice numbers its sites


def _chain_pairs(idx, periodic, rows=None):
    """(E, 2) 1-2 and 1-3 pairs along the first axis of idx[X][Y][Z]; rows: mask over [Y][Z] of the lattice rows that are bonded."""
    out = []
    for step in (1, 2):
        a, b = (idx, np.roll(idx, -step, axis=0)) if periodic else (idx[:-step], idx[step:])
        keep = np.ones(a.shape, dtype=bool) if rows is None else np.broadcast_to(rows[None], a.shape)
        out.append(np.stack([a[keep], b[keep]], axis=1))
    return np.concatenate(out)


def _around(site, offsets):
    idx = _idx()
    c = np.array(site)
    assert all(((c + o >= 0) & (c + o < LJ_M)).all() for o in offsets)
    return np.array([[idx[tuple(c)], idx[tuple(c + o)]] for o in offsets])


@functools.lru_cache(maxsize=None)
def topology(name, box):
    """(given, unique): the (E, 2) int32 pairs as the test hands them to nl_set_exclusions -- for the chains in both orders and
    with duplicates -- and the distinct unordered pairs (i < j), sorted."""
    assert name in TOPOLOGIES
    periodic = bool(LJ_BOXES[box][1] & 1)
    idx = _idx()
    if name == "chains":
        p = _chain_pairs(idx, periodic)
        given = np.concatenate([p, p[::3, ::-1], p[::7]])
    else:
        yz = np.arange(LJ_M * LJ_M).reshape(LJ_M, LJ_M)
        bonded = yz % 4 != 3
        assert not bonded[HUB[1], HUB[2]] and not bonded[EIGHT[1], EIGHT[2]] and not bonded[NINE[1], NINE[2]]
        cube = [np.array(o) for o in np.ndindex(3, 3, 3)]
        all26 = [o - 1 for o in cube if tuple(o) != (1, 1, 1)]
        corners = [o for o in all26 if np.abs(o).sum() == 3]
        given = np.concatenate([_chain_pairs(idx, periodic, bonded), _around(HUB, all26), _around(EIGHT, corners),
                                _around(NINE, corners + [np.array([1, 0, 0])])])
    given = np.ascontiguousarray(given.astype(np.int32))
    lo, hi = given.min(axis=1), given.max(axis=1)
    unique = np.unique(np.stack([lo, hi], axis=1).astype(np.int64), axis=0)
    assert (unique[:, 0] < unique[:, 1]).all() and (len(given) > len(unique) if name == "chains" else len(given) == len(unique))
    given.setflags(write=False), unique.setflags(write=False)
    return given, unique


def csr(unique, n):
    """(offsets[n + 1], ids): the symmetric, per-row ascending table of nl_get_exclusions from the distinct pairs."""
    a = np.concatenate([unique[:, 0], unique[:, 1]])
    b = np.concatenate([unique[:, 1], unique[:, 0]])
    order = np.lexsort((b, a))
    return np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))]).astype(np.int32), b[order].astype(np.int32)


def ordered(unique):
    """(I, J): every entry of the table, both directions of every pair."""
    return np.concatenate([unique[:, 0], unique[:, 1]]), np.concatenate([unique[:, 1], unique[:, 0]])


@functools.lru_cache(maxsize=None)
def excl_tab(nk=NKX, r_min=R_MIN, r_max=R_MAX):
    """(K, C) of the excluded-pair table."""
    return coulomb.ewald_excluded(ALPHA, r_min, r_max, nk, prefactor=PREFACTOR)


def assert_in_range(q, box6, mask, unique, r_min=R_MIN, r_max=R_MAX):
    """Every pair of the topology lies inside (r_min, r_max), a 2^-10 of r^2 away from either end; returns (min r, max r)."""
    I, J = ordered(unique)
    d = lj_list_separations(q, I, J, box6, mask)
    r2 = (d * d).sum(axis=1)
    assert r2.min() > r_min ** 2 * (1 + 2.0 ** -10) and r2.max() < r_max ** 2 * (1 - 2.0 ** -10), (r2.min() ** 0.5, r2.max() ** 0.5)
    return float(r2.min() ** 0.5), float(r2.max() ** 0.5)


# -------------------------------------------------------------------------------------------------------- reference
def excl_reference(q, box6, mask, K, C, r_min, r_max, chg, unique):
    """(forces (want[n, 4], S[n, 4]), totals (want[8], S[7])) of the rule of nl_set_coul_excl_table in float64: a direct loop
    over the table's pairs, no list and no O(N^2) sweep; the separation is the nearest image, folded in long double
    (tests.util lj_list_separations).  A pair outside [r_min, r_max) is NaN.  S: the uncancelled magnitudes
    |q_i q_j| (|V_k| + |V_k+1| + |dV_k| r2 / D), the third term the conditioning of s on the rounding of r2.  The totals are
    summed in long double, every pair once."""
    n = len(q)
    chg = np.asarray(chg, dtype=np.float64)
    I, J = ordered(unique)
    d = lj_list_separations(q, I, J, box6, mask)
    r2 = (d * d).sum(axis=1)
    kc, cc, _ = coulomb.interpolate(K, C, r_min, r_max, r2)
    ok = (r2 >= float(r_min) ** 2) & (r2 < float(r_max) ** 2)
    qq = chg[I] * chg[J]
    fc, ec = np.where(ok, qq * kc, np.nan), np.where(ok, qq * cc, np.nan)
    nk = len(K)
    D = pair_table.spacing(r_min, r_max, nk)
    k = np.clip(((r2 - float(r_min) ** 2) / D).astype(np.int64), 0, nk - 2)
    mf, mu = (np.abs(qq) * (np.abs(t[k]) + np.abs(t[k + 1]) + np.abs(t[k + 1] - t[k]) * r2 / D) for t in (K, C))
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fc * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=mf * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=0.5 * ec, minlength=n)
    S[:, 3] = np.bincount(I, weights=0.5 * mu, minlength=n)
    assert np.finfo(np.longdouble).nmant >= 63, "excl_reference needs an extended-precision long double"
    fl, el, dl = fc.astype(np.longdouble), ec.astype(np.longdouble), d.astype(np.longdouble)
    n_in = np.nan if np.isnan(fc).any() else float(len(unique))
    ww = np.array([float(0.5 * (fl * dl[:, a] * dl[:, b]).sum()) for a, b in _AB] + [float(0.5 * el.sum()), n_in])
    if np.isnan(n_in):
        ww[:] = np.nan
    SW = np.array([0.5 * (mf * np.abs(d[:, a] * d[:, b])).sum() for a, b in _AB] + [0.5 * mu.sum()])
    return (want, S), (ww, SW)


@functools.lru_cache(maxsize=None)
def ref(box, drift, topo, kind="salt"):
    box6, mask = LJ_BOXES[box]
    return excl_reference(_input(box, drift), box6, mask, *excl_tab(), R_MIN, R_MAX, charges(kind), topology(topo, box)[1])


@functools.lru_cache(maxsize=None)
def moved_ref(box, topo, kind="salt"):
    box6, mask = LJ_BOXES[box]
    return excl_reference(_moved(box)[0], box6, mask, *excl_tab(), R_MIN, R_MAX, charges(kind), topology(topo, box)[1])


def weakest(K, C, r_max, q_min):
    """(force component, energy) the weakest single pair at r_max gives a particle: |q_i q_j| |K(r_max)| r_max / sqrt(3) and
    |q_i q_j| |C(r_max)| / 2 for charges no smaller than q_min."""
    return q_min ** 2 * abs(K[-1]) * r_max / np.sqrt(3.0), 0.5 * q_min ** 2 * abs(C[-1])


# -------------------------------------------------------------------------------------------------------- emulation
def excl_emulate_pairs(q, box6, mask, K, C, r_min, r_max, chg, T, I, J, defect=None):
    """lj_image (tests.util emulate_pairs) and cx_row_pairs (csrc/nl_coul_excl.inc) in the position type T over the entries
    (I, J): one rounding per operation, no FMA.  Returns (dx, dy, dz, fx, fy, fz, ec) in T.  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    T = np.dtype(T).type
    dx, dy, dz = emulate_pairs(q, box6, 0 if defect == "the plain difference" else mask, 1.0, 1.0, 1.0, T, (I, J))[:3]
    r2 = dx * dx + dy * dy + dz * dz
    Kt, dKt, Ct, dCt, x0, xc, iD = table_device_form(K, C, r_min, r_max, T)
    if defect == "C and K swapped":
        Kt, dKt, Ct, dCt = Ct, dCt, Kt, dKt
    inn = (r2 >= x0) & (r2 < xc)
    s = (r2 - x0) * iD
    k = np.where(inn, np.minimum(np.where(inn, s, T(0)).astype(np.int32), Kt.shape[1] - 2), 0)
    t = s - k.astype(T)
    qt = np.asarray(chg, dtype=np.float64).astype(T)
    qq = qt[J] if defect == "qj for qq" else qt[I] * qt[J]
    fc = np.where(inn, qq * (Kt[0, k] + t * dKt[0, k]), T(np.nan))
    ec = np.where(inn, qq * (Ct[0, k] + t * dCt[0, k]), T(np.nan))
    out = (dx, dy, dz, fc * dx, fc * dy, fc * dz, ec)
    assert all(v.dtype == np.dtype(T) for v in out)
    return out


def excl_emulate(n, I, vals, rng, defect=None):
    """The row body of k_coul_excl_forces over excl_emulate_pairs' values: f = {fx, fy, fz, ec / 2} summed per particle in T,
    every particle's terms in a random order (the kernel's order is one of many).  Returns f[n, 4] in T."""
    _, _, _, fx, fy, fz, ec = vals
    T = fx.dtype.type
    term = np.stack([fx, fy, fz, np.zeros_like(ec) if defect == "no term in pe" else T(0.5) * ec], axis=1)
    assert term.dtype == fx.dtype
    return _sum_rows(n, I, term, rng)


def excl_virial_emulate(n, I, vals, rng, defect=None, nblk=256):
    """k_coul_excl_virial and k_virial_reduce over excl_emulate_pairs' values with the kernels' own summation tree: the six
    products and the energy in T, converted to double (exact); row r goes to block (r // 32) mod nblk, group r mod 32 of it, its
    entries (in a random order) to the 8 lanes of the group in turn, every lane adds its terms one after the other; then the
    butterfly of the wave, waves ((0 + 1) + 2) + 3, the partials of the blocks by tests.util_table _block_sum, and the weight
    1/2.  nblk: NL_COUL_EXCL_BLOCKS.  Returns the 7 sums and n_in."""
    dx, dy, dz, fx, fy, fz, ec = vals
    terms = [fx * dx, fy * dy, fz * dz, fx * dy, fx * dz, fy * dz, ec]
    assert all(t.dtype == dx.dtype for t in terms)
    w = 1.0 if defect == "an entry with weight 1 in the totals" else 0.5
    if any(np.isnan(t).any() for t in terms):
        return np.full(8, np.nan)
    nblk = min((n + 31) // 32, nblk)
    order = np.lexsort((rng.random(len(I)), I))
    Is = I[order]
    pos = np.arange(len(Is)) - np.searchsorted(Is, np.arange(n))[Is]  # the entry's place in its row
    thread = ((Is // 32) % nblk) * 256 + (Is % 32) * 8 + pos % 8
    key = np.lexsort((pos // 8, (Is // 32) // nblk, thread))  # a lane's terms in the order it meets them
    out = np.zeros(7)
    for c, t in enumerate(terms):
        acc = np.bincount(thread[key], weights=t.astype(np.float64)[order][key], minlength=nblk * 256)  # (adds in order)
        acc = acc.reshape(nblk, 4, 64)
        while acc.shape[2] > 1:  # wave_sum
            acc = acc[:, :, :acc.shape[2] // 2] + acc[:, :, acc.shape[2] // 2:]
        part = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
        out[c] = w * _block_sum(part)[0]
    return np.concatenate([out, [w * len(dx)]])


# ------------------------------------------------------------------------------------------------- the 10 976-particle grid
@functools.lru_cache(maxsize=None)
def big_chains():
    """The chains on tests.consumer_util _big (the "xyz" lattice tiled 2 x 2 x 1, tile ix * 2 + iy): 1-2 and 1-3 pairs along x
    over both tiles, periodic.  Returns the distinct pairs."""
    idx = _idx()
    big = np.concatenate([np.concatenate([idx + (ix * 2 + iy) * N for iy in range(2)], axis=1) for ix in range(2)], axis=0)
    assert big.shape == (2 * LJ_M, 2 * LJ_M, LJ_M) and len(np.unique(big)) == 4 * N
    p = _chain_pairs(big, True)
    return np.unique(np.stack([p.min(axis=1), p.max(axis=1)], axis=1).astype(np.int64), axis=0)


"""Inputs and handle helpers that the consumer tests share (test_lj_consumer, test_lj_virial, test_pair_histogram,
test_pair_table, test_eam, test_sw, test_slab_consumers): the 14^3 jittered lattice in its two forms, the tables sampled on it,
and the handle of a box of LJ_BOXES.  Nothing here calls a consumer; the contract the consumers share is tests.consumer_contract.

Two families of inputs, both n = 2744, SEED 11, the boxes and position states of CASES:
  * lj_*: tests.util lj_lattice with every rc_force of PARS among its cuts (the Lennard-Jones forces, totals, histogram);
  * table_*: lj_lattice with cuts = (R_MIN, R_MAX), the grid of the tabulated potentials (pair table, EAM, Stillinger-Weber).
"""
import functools

import numpy as np

from md_neighbor_list_amd import pair_table, rdf
from tests.util import (LJ_A, LJ_BOXES, LJ_L, LJ_M, lj_band_particles, lj_drift, lj_lattice, lj_pairs, lj_type_params, lj_wrap)
from tests.util_table import lj, morse
from tests.virial_util import virial_reference

SEED = 11
N = LJ_M ** 3
DTYPES = [np.float32, np.float64]
CASES = [("open", False), ("xy", False), ("xy", True), ("xyz", False), ("xyz", True), ("tilt", False), ("tilt", True),
         ("hex", False), ("hex", True)]

# the Lennard-Jones family
RCF = 2.5
RC_LISTS = (2.5, 3.4, 3.6)
PARS = ("scalar", "typed3", "typed32")
# what the emulation that fixes c runs over: every box and mask in the box and drifted, scalars and both type tables
EMULATED = [("xyz", False, "scalar"), ("xyz", True, "scalar"), ("tilt", False, "scalar"), ("tilt", True, "scalar"),
            ("xy", True, "scalar"), ("hex", True, "scalar"), ("open", False, "scalar"), ("xyz", True, "typed3"),
            ("tilt", True, "typed32")]
NBLK_VIRIAL = 2048  # NL_VIRIAL_BLOCKS of include/nl_hip.h: the most blocks of 4 waves k_lj_virial is launched with
BIG_BOX = ((2 * LJ_L, 2 * LJ_L, LJ_L, 0.0, 0.0, 0.0), 7)
# the histogram's designed inputs, box: (r_max, nbins); every edge, 2.5 and 3.4 are cuts of its lattice.  ("hex" is the "xyz" shape on
# the sheared film.)
HIST_INPUTS = {"xyz": (2.5, 50), "tilt": (3.0, 64), "open": (2.5, 7), "xy": (3.4, 128), "hex": (2.5, 50)}

# the table family
R_MIN, R_MAX = 0.85, 2.5
NK = 1024


def _torch():
    import torch

    return torch


def _tdt(dtype):
    return _torch().float32 if dtype == np.float32 else _torch().float64


def _handle(box, dtype, full, rc, off=0, images=False):
    torch = _torch()
    from md_neighbor_list_amd import NeighListGPU

    box6, mask = LJ_BOXES[box]
    axes = tuple(bool(mask >> a & 1) for a in range(3))
    nl = NeighListGPU(rc, *box6[:3], dtype=torch.float32 if dtype == np.float32 else torch.float64, full_list=full,
                      minimum_image=axes if mask else False, tilt=box6[3:])
    if off:
        nl.set_offset_width(off)
    if images:
        nl.set_pair_images(True)
    return nl


@functools.lru_cache(maxsize=None)
def _bonds():
    """1-2 bonds along x of the lattice: every site with its +x neighbour, periodic."""
    idx = np.arange(N).reshape(LJ_M, LJ_M, LJ_M)
    return np.stack([idx.ravel(), np.roll(idx, -1, axis=0).ravel()], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------- the Lennard-Jones family's inputs
@functools.lru_cache(maxsize=None)
def _lj_par(name, rc_list=3.4):
    """(types, rc_ab, eps, sig, rcf) of a parameter set; scalars: (None, None, 1, 1, 2.5)."""
    if name == "scalar":
        return None, None, 1.0, 1.0, RCF
    return lj_type_params(int(name[5:]), rc_list)


@functools.lru_cache(maxsize=None)
def _lj_cuts():
    """Every rc_force any case uses: the lattice keeps its pairs out of the band around each."""
    c = {RCF}
    for name in PARS[1:]:
        c |= set(np.unique(_lj_par(name)[4]).tolist()) - {0.0}
    return tuple(sorted(c))


@functools.lru_cache(maxsize=None)
def _lj_input(box, drift, shift=False):
    """[n, 4] float64 holding float32 values.  shift: the lattice moved by a / 2 and wrapped, so that particles sit on
    both sides of every periodic face (the skin tests)."""
    box6, mask = LJ_BOXES[box]
    if drift:
        q = lj_drift(_lj_input(box, False, shift), SEED + 1, box)
        q[:, :3] = q[:, :3].astype(np.float32)
        q.setflags(write=False)
        return q
    q = lj_lattice(SEED, box, cuts=_lj_cuts()) if not shift else _lj_input(box, False).copy()
    if shift:
        q[:, :3] = lj_wrap(q[:, :3] - 0.5 * LJ_A * np.array([mask & 1, mask >> 1 & 1, mask >> 2 & 1]), box6, mask)
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _lj_pairs(box, drift, shift=False):
    box6, mask = LJ_BOXES[box]
    p = lj_pairs(_lj_input(box, drift, shift), box6, mask, max(RC_LISTS))
    assert not len(lj_band_particles(None, box6, mask, _lj_cuts(), 2.0 ** -17, pairs=p)), "a pair in the band of a cut-off"
    return p


@functools.lru_cache(maxsize=None)
def _lj_moved(box, step=0.03, seed=21):
    """The shifted lattice of `box` with every particle moved by up to `step` per axis (far below skin / 2 = 0.2): particles
    leave through the faces, pairs cross rc_force both ways, none ends in the band of a cut-off."""
    box6, mask = LJ_BOXES[box]
    q0 = _lj_input(box, False, True)
    rng = np.random.default_rng(seed)
    q = q0.copy()
    todo = np.arange(N)
    for _ in range(20):
        q[todo, :3] = (q0[todo, :3] + rng.uniform(-step, step, size=(len(todo), 3))).astype(np.float32)
        todo = lj_band_particles(q, box6, mask, _lj_cuts(), 2.0 ** -15, rows=todo)
        if not len(todo):
            break
    assert not len(todo)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _lj_moved_pairs(box):
    box6, mask = LJ_BOXES[box]
    return lj_pairs(_lj_moved(box), box6, mask, RCF)


def _lj_forces(q, box, dtype, full, rc, par, off=0, stride=4, exclusions=None):
    """(handle, device positions, forces on the host) of one build and one blocking consumer call."""
    torch = _torch()
    n = len(q)
    nl = _handle(box, dtype, full, rc, off)
    nl.Initialize(n)
    types, _, eps, sig, rcf = _lj_par(par, rc)
    if types is not None:
        nl.set_type_cutoffs(types, _lj_par(par, rc)[1])
    if exclusions is not None:
        nl.set_exclusions(exclusions, n)
    qd = torch.from_numpy(np.ascontiguousarray(q[:, :stride].astype(dtype))).cuda()
    nl.MakeNeighList(qd, n)
    if off:
        assert nl.build_info()["offset_bits"] == off
    if types is not None:
        nl.set_lj_type_params(eps, sig, rcf)
        f = nl.lj_forces_typed(qd)
    else:
        f = nl.lj_forces(qd, 1.0, 1.0, rc_force=RCF)
    return nl, qd, f.cpu().numpy()


def _dimers(dtype, box6, mask, seed=5):
    """Two-particle molecules on a 6^3 grid of spacing 10.5 (L = 63), on grid points i * 10.5: those with i = 0 straddle a
    face, two or three of them an edge or the corner.  Coordinates are multiples of 2^-16 (fp32) / 2^-45 (fp64), so the
    separations and their folds are exact in the position type and the comparison is of lj_pair alone.  Returns
    (q[2 m, 4] with partners adjacent, group per dimer): 0 = r in [0.9, rc_force (1 - 2^-10)], 1 = below the band
    rc_force (1 - k s), 2 = above it (4 <= k <= 64; s = 2^-20 for fp32, 2^-49 for fp64), 3 = coincident."""
    rng = np.random.default_rng(seed)
    grid, s = (2.0 ** -16, 2.0 ** -20) if dtype == np.float32 else (2.0 ** -45, 2.0 ** -49)
    g = np.stack(np.meshgrid(*(np.arange(6),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    if not mask:
        g = g + 0.5  # (an open box: every molecule inside)
    mid = g * 10.5
    m = len(mid)
    group = rng.permutation(np.arange(m) % 8)
    group = np.where(group < 4, 0, np.where(group < 6, 1, np.where(group == 6, 2, 3)))
    u = rng.normal(size=(m, 3))
    u = np.where(np.abs(u) < 0.2, 0.2, u)  # (every component takes part: a molecule on a face crosses it)
    u /= np.linalg.norm(u, axis=1)[:, None]
    k = rng.uniform(12.0, 56.0, size=m)
    r = np.where(group == 0, rng.uniform(0.9, RCF * (1 - 2.0 ** -10), size=m),
                 np.where(group == 1, RCF * (1 - k * s), np.where(group == 2, RCF * (1 + k * s), 0.0)))
    p1 = np.round((mid - 0.5 * r[:, None] * u) / grid) * grid
    p2 = np.round((p1 + r[:, None] * u) / grid) * grid
    p2[group == 3] = p1[group == 3]
    got = np.sqrt(((p2 - p1) ** 2).sum(axis=1)) / RCF - 1.0
    assert np.all((got[group == 1] <= -4 * s) & (got[group == 1] >= -64 * s))
    assert np.all((got[group == 2] >= 4 * s) & (got[group == 2] <= 64 * s))
    q = np.zeros((2 * m, 4))
    q[0::2, :3], q[1::2, :3] = p1, p2
    q[:, :3] = lj_wrap(q[:, :3], box6, mask)
    return q, group, np.flatnonzero((g >= 1).all(axis=1))


@functools.lru_cache(maxsize=None)
def _big():
    """The "xyz" lattice tiled 2 x 2 x 1 and rounded to float32 again (coordinates in [16, 32) lose a bit): n = 10976 rows
    for at most 4 NBLK_VIRIAL = 8192 waves, so waves take a second row and the last turn is ragged.  (q, reference)"""
    base = _lj_input("xyz", False)
    q = np.concatenate([base + np.array([ix * LJ_L, iy * LJ_L, 0.0, 0.0]) for ix in range(2) for iy in range(2)])
    q[:, :3] = q[:, :3].astype(np.float32)
    box6, mask = BIG_BOX
    pairs = lj_pairs(q, box6, mask, RCF * (1 + 2.0 ** -16))
    assert not len(lj_band_particles(None, box6, mask, (RCF,), 2.0 ** -17, pairs=pairs)), "a pair in the band of the cut-off"
    q.setflags(write=False)
    return q, virial_reference(q, box6, mask, 1.0, 1.0, RCF, pairs=pairs)


# --------------------------------------------------------------------------------------------- the table family's inputs
def _pair_tab(nt, r_min, r_max, nk):
    """The pair tables of _tab ("morse", "typed3") on another grid."""
    if nt == 1:
        return pair_table.sample(*morse(), r_min, r_max, nk)
    rows = [pair_table.sample(*morse(De=1.0 + 0.2 * (s % 5), a=1.5, r0=1.05 + 0.03 * (s % 6)), r_min, r_max, nk) for s in range(rdf.nslots(nt))]
    F, U = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    F[rdf.slot(0, nt - 1, nt)] = U[rdf.slot(0, nt - 1, nt)] = 0.0
    return F, U


@functools.lru_cache(maxsize=None)
def _tab(name, nk=NK):
    """(F, U, types, rc_ab(rc_list)) of a table on the grid (R_MIN, R_MAX, nk).  typed3: a Morse potential per pair of 3
    types, the slot of the pair (0, 2) -- which the type table leaves out of the list -- zero."""
    if name in ("morse", "lj"):
        F, U = pair_table.sample(*(morse() if name == "morse" else lj()), R_MIN, R_MAX, nk)
        return F, U, None, None
    nt = int(name[5:])
    types = lj_type_params(nt, 3.4)[0]
    rows = [pair_table.sample(*morse(De=1.0 + 0.2 * (s % 5), a=1.5, r0=1.05 + 0.03 * (s % 6)), R_MIN, R_MAX, nk) for s in range(rdf.nslots(nt))]
    F, U = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    F[rdf.slot(0, nt - 1, nt)] = U[rdf.slot(0, nt - 1, nt)] = 0.0

    def rc_ab(rc_list):
        rc = np.full((nt, nt), float(rc_list))
        rc[0, nt - 1] = rc[nt - 1, 0] = 0.0
        return rc

    return F, U, types, rc_ab


@functools.lru_cache(maxsize=None)
def _table_input(box, drift):
    """[n, 4] float64 holding float32 values."""
    q = lj_drift(_table_input(box, False), SEED + 1, box) if drift else lj_lattice(SEED, box, cuts=(R_MIN, R_MAX))
    q[:, :3] = q[:, :3].astype(np.float32)
    q.setflags(write=False)
    return q


def _off_the_band(q, box6, mask, pairs):
    return not len(lj_band_particles(None, box6, mask, (R_MIN, R_MAX), 2.0 ** -17, pairs=pairs))


@functools.lru_cache(maxsize=None)
def _table_pairs(box, drift):
    box6, mask = LJ_BOXES[box]
    p = lj_pairs(_table_input(box, drift), box6, mask, R_MAX * (1 + 2.0 ** -16))
    assert _off_the_band(None, box6, mask, p), "a pair in the band of r_max or r_min"
    return p


@functools.lru_cache(maxsize=None)
def _table_moved(box, seed=21, step=0.03):
    """The lattice of `box` with every particle moved by up to `step` per axis (far below skin / 2), none into the band."""
    box6, mask = LJ_BOXES[box]
    q0 = _table_input(box, False)
    rng = np.random.default_rng(seed)
    q, todo = q0.copy(), np.arange(N)
    for _ in range(20):
        q[todo, :3] = (q0[todo, :3] + rng.uniform(-step, step, size=(len(todo), 3))).astype(np.float32)
        todo = lj_band_particles(q, box6, mask, (R_MIN, R_MAX), 2.0 ** -15, rows=todo)
        if not len(todo):
            break
    assert not len(todo)
    q.setflags(write=False)
    return q, lj_pairs(q, box6, mask, R_MAX * (1 + 2.0 ** -16))

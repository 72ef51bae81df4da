"""Shared helpers of the test-suite."""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_names(dup=None):
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
    if dup is None:
        return names
    return [n for n in names if n.startswith("dup_") == bool(dup)]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def canonical_csr(key_pointer, sorted_list):
    """Per-particle ascending partners (make_list.cpp:120-128) with numpy only."""
    kp = np.asarray(key_pointer, dtype=np.int64)
    lst = np.asarray(sorted_list, dtype=np.int64)
    n = len(kp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(kp))
    if len(lst) and int(lst.min()) >= 0 and int(lst.max()) < 2**31 and n < 2**31:
        key = (rows << 32) | lst  # one 64-bit key per entry: a plain sort instead of a two-key lexsort (4 x faster)
        key.sort()
        return (key & 0xFFFFFFFF).astype(np.int32)
    order = np.lexsort((lst, rows))
    return lst[order].astype(np.int32)


def gpu_build(q, rc, box, sync=True):
    """Runs the HIP path through the C ABI; returns (number_of_partners, key_pointer, sorted_list) on the host."""
    import torch

    from md_neighbor_list_amd import NeighListGPU

    dt = torch.float32 if q.dtype == np.float32 else torch.float64
    nl = NeighListGPU(rc, box[0], box[1], box[2], dtype=dt)
    nl.Initialize(len(q))
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nl.MakeNeighList(qd, len(q), sync=sync)
    if not sync:
        nl.synchronize()
    nop = nl.half_number_of_partners().cpu().numpy()
    kp = nl.key_pointer().cpu().numpy()
    sl = nl.sorted_list().cpu().numpy()
    return nl, nop, kp, sl


# ------------------------------------------------------------------------------------------ Lennard-Jones consumer
# The contract the consumer is tested against (tests/test_lj_consumer.py): every component of
# every particle within LJ_C * u * S of an O(N^2) float64 sum, S the uncancelled magnitudes of that component's pair
# terms and u the unit roundoff of the position type.  LJ_C is 4 x the largest ratio a float32 emulation of lj_pair
# (lj_emulate, random summation order) reaches on the lattice inputs; test_emulation_gives_c recomputes it.
LJ_C = 51.2


def lj_fold(d, box6, mask):
    """Folds separations d[k, 3] (float64, in place) on the axes of mask in z, y, x order with the tilts: the rule of
    include/nl_hip.h (nl_set_box)."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box6)
    if mask & 4:
        k = np.rint(d[:, 2] / Lz)
        d[:, 2] -= k * Lz
        d[:, 1] -= k * yz
        d[:, 0] -= k * xz
    if mask & 2:
        k = np.rint(d[:, 1] / Ly)
        d[:, 1] -= k * Ly
        d[:, 0] -= k * xy
    if mask & 1:
        d[:, 0] -= np.rint(d[:, 0] / Lx) * Lx
    return d


def lj_list_separations(q, rows, cols, box6, mask):
    """d = r_rows - r_cols at the image, for the pairs of a list, to float64 accuracy of the *folded* separation.  A float64
    difference of float64 coordinates across a face is rounded at the size of L before the fold takes L off: half an ulp
    of L is 16 u of a separation near 1 at L = 32, and 14 times that in an r^-13 force -- more than the bound of check_lj,
    while the consumer folds the exact difference.  So the difference and the fold are taken in long double (64-bit
    significand) and only the folded result is rounded.  float32 coordinates need none of this and get it all the same."""
    assert np.finfo(np.longdouble).nmant >= 63, "lj_list_separations needs an extended-precision long double"
    p = np.asarray(q)[:, :3].astype(np.longdouble)
    return lj_fold(p[rows] - p[cols], box6, mask).astype(np.float64)


def lj_pairs(q, box6, mask, rmax, fold=lj_fold, rows=None):
    """Every ordered pair (i, j), i != j, with folded r < rmax by an O(N^2) float64 sweep: (I, J, d = r_i - r_j, raw d).
    Uses no list, the library's or the oracle's.  rows: only the pairs with i in rows."""
    p = np.asarray(q)[:, :3].astype(np.float64)
    n = len(p)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    out = [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 3)))]
    step = max(1, (1 << 20) // max(n, 1))
    for i0 in range(0, len(rows), step):
        ii = rows[i0:i0 + step]
        raw = (p[ii, None, :] - p[None, :, :]).reshape(-1, 3)
        d = fold(raw.copy(), box6, mask)
        r2 = np.einsum("ij,ij->i", d, d)
        k = np.flatnonzero(r2 < rmax * rmax)
        i, j = ii[k // n], k % n
        keep = i != j
        out.append((i[keep], j[keep], d[k[keep]], raw[k[keep]]))
    return tuple(np.concatenate([o[c] for o in out]) for c in range(4))


def _lj_par(v, types, I, J):
    v = np.asarray(v, dtype=np.float64)
    return v if v.ndim == 0 else v[types[I], types[J]]


def lj_reference(q, box6, mask, eps, sig, rcf, types=None, exclusions=None, pairs=None):
    """Truncated Lennard-Jones forces and per-particle energies by an O(N^2) float64 sum: (want[n, 4], S[n, 4]).
    A pair enters iff 0 < r^2 < rcf_ab^2: F_i += 24 eps (2 s12 - s6) / r^2 d, pe_i += 1/2 4 eps (s12 - s6).  S holds the
    uncancelled magnitudes, sum 24 eps (2 s12 + s6) / r^2 |d_c| and sum 2 eps (s12 + s6): the plus signs keep the bound
    of check_lj meaningful near the force zero at r = 2^(1/6) sigma.  eps, sig, rcf: scalars, or matrices read at
    [type of i][type of j].  exclusions: (E, 2) pairs left out.  pairs: lj_pairs(q, box6, mask, >= max rcf) to reuse."""
    n = len(q)
    types = None if types is None else np.asarray(types, dtype=np.int64)
    I, J, d, _ = lj_pairs(q, box6, mask, float(np.max(rcf))) if pairs is None else pairs
    e, s, c = (_lj_par(v, types, I, J) for v in (eps, sig, rcf))
    r2 = (d * d).sum(axis=1)
    keep = (r2 > 0) & (r2 < c * c)
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keys = np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]])
        keep &= ~np.isin(I * n + J, keys)
    I, d, r2 = I[keep], d[keep], r2[keep]
    e, s = (v if v.ndim == 0 else v[keep] for v in (e, s))
    s6 = (s * s / r2) ** 3
    s12 = s6 * s6
    fr = 24.0 * e * (2.0 * s12 - s6) / r2
    fa = 24.0 * np.abs(e) * (2.0 * s12 + s6) / r2
    want, S = np.zeros((n, 4)), np.zeros((n, 4))
    for a in range(3):
        want[:, a] = np.bincount(I, weights=fr * d[:, a], minlength=n)
        S[:, a] = np.bincount(I, weights=fa * np.abs(d[:, a]), minlength=n)
    want[:, 3] = np.bincount(I, weights=2.0 * e * (s12 - s6), minlength=n)
    S[:, 3] = np.bincount(I, weights=2.0 * np.abs(e) * (s12 + s6), minlength=n)
    return want, S


def lj_unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def lj_ratio(got, want, S, dtype):
    """|got - want| / (u S) per particle and column (0 where both vanish, inf where only the bound does or got is NaN)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    den = lj_unit(dtype) * S
    r = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def check_lj(got, want, S, dtype, c=LJ_C, rows=None):
    """Asserts |got - want| <= c u S for every particle (of rows) and every column separately."""
    r = lj_ratio(got, want, S, dtype)
    if rows is not None:
        r = r[rows]
    i, col = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r[i, col] <= c, (f"particle {i if rows is None else np.arange(len(want))[rows][i]}, column {'xyze'[col]}: "
                            f"|got - want| = {r[i, col]:.4g} u S, allowed {c:g} (worst per column {r.max(axis=0)})")


def emulate_pairs(q, box6, mask, eps, sig, rcf, T, pairs, types=None):
    """lj_image and lj_pair (csrc/nl_consumer.inc) in the position type T with numpy over the ordered pairs (I, J) of
    `pairs`: one rounding per operation and no FMA beyond the kernel's own, up to the pair's values
    (dx, dy, dz, fx, fy, fz, pe, in) in T.  What the consumer's kernels do with them: lj_emulate, tests.virial_util
    virial_emulate."""
    T = np.dtype(T).type
    I, J = pairs[0], pairs[1]
    p = np.asarray(q)[:, :3].astype(T)
    a, b = p[I], -p[J]
    d = a + b
    bv = d - a
    lo = (a - (d - bv)) + (b - bv)  # TwoSum: d + lo = r_i - r_j exactly
    dx, dy, dz = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
    L = [T(box6[a]) if mask >> a & 1 else T(0) for a in range(3)]
    xy, xz, yz = (T(v) for v in box6[3:])

    def fnma(k, m, v):  # fma(-k, m, v): one rounding
        return (v.astype(np.longdouble) - k.astype(np.longdouble) * np.longdouble(m)).astype(T)

    def sub_kl(k, m, v, lo):  # sub_kl of the kernel: (v, lo) -= k m, the step's rounding error kept in lo
        pr = k * m
        pe = (k.astype(np.longdouble) * np.longdouble(m) - pr.astype(np.longdouble)).astype(T)  # fma(k, m, -pr): exact
        s = v - pr
        bv = s - v
        return s, lo + (((v - (s - bv)) - (pr + bv)) - pe)

    if mask:
        iL = [T(1) / v if v > 0 else T(0) for v in L]
        kz = np.rint(dz * iL[2])
        ky = np.rint((dy - kz * yz) * iL[1])
        kx = np.rint(((dx - kz * xz) - ky * xy) * iL[0])
        dz = fnma(kz, L[2], dz)
        lx, ly = lo[:, 0], lo[:, 1]
        if xy != 0 or xz != 0 or yz != 0:  # the tilted instances
            dy, ly = sub_kl(ky, L[1], dy, ly)
            dy, ly = sub_kl(kz, yz, dy, ly)
            dx, lx = sub_kl(kx, L[0], dx, lx)
            dx, lx = sub_kl(ky, xy, dx, lx)
            dx, lx = sub_kl(kz, xz, dx, lx)
        else:
            dy, dx = fnma(ky, L[1], dy), fnma(kx, L[0], dx)
        dx, dy, dz = dx + lx, dy + ly, dz + lo[:, 2]
    types = None if types is None else np.asarray(types, dtype=np.int64)
    e, s, c = (_lj_par(v, types, I, J) for v in (eps, sig, rcf))
    eps4, sig2, rcf2 = (4.0 * e).astype(T), (s * s).astype(T), (c * c).astype(T)  # (double products rounded once: the host's)
    r2 = dx * dx + dy * dy + dz * dz
    inn = (r2 < rcf2) & (r2 > 0)
    safe = np.where(inn, r2, T(1))
    ir2 = np.where(inn, sig2 / safe, T(0))
    s6 = ir2 * ir2 * ir2
    fr = np.where(inn, T(6) * eps4 * (s6 + s6 - T(1)) * s6 / safe, T(0))
    out = (dx, dy, dz, fr * dx, fr * dy, fr * dz, eps4 * (s6 - T(1)) * s6, inn)
    assert all(v.dtype == np.dtype(T) for v in out[:7])
    return out


def lj_emulate(q, box6, mask, eps, sig, rcf, T, rng, pairs, types=None):
    """The row body of k_lj over emulate_pairs' values, f = {fx, fy, fz, pe / 2} summed per particle in T: every particle's
    terms are added in a random order, as the half list's atomics and the wave reduction fix none.  Returns f[n, 4] in T."""
    T = np.dtype(T).type
    n, I = len(q), pairs[0]
    _, _, _, fx, fy, fz, pe, _ = emulate_pairs(q, box6, mask, eps, sig, rcf, T, pairs, types=types)
    term = np.stack([fx, fy, fz, T(0.5) * pe], axis=1)
    assert term.dtype == np.dtype(T)
    order = np.lexsort((rng.random(len(I)), I))
    Is, term = I[order], term[order]
    start = np.searchsorted(Is, np.arange(n))
    rank = np.arange(len(Is)) - start[Is]
    f = np.zeros((n, 4), dtype=T)
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        f[Is[sel]] += term[sel]
    return f


# The inputs of tests/test_lj_consumer.py: a jittered simple-cubic lattice whose spacing and box are exact in float32.
LJ_A, LJ_M = 1.125, 14
LJ_L = LJ_A * LJ_M  # 15.75
LJ_BOXES = {  # name: (box6, mask)
    "open": ((LJ_L, LJ_L, LJ_L, 0.0, 0.0, 0.0), 0),
    "xy": ((LJ_L, LJ_L, LJ_L, 0.0, 0.0, 0.0), 3),
    "xyz": ((LJ_L, LJ_L, LJ_L, 0.0, 0.0, 0.0), 7),
    "tilt": ((LJ_L, LJ_L, LJ_L, 2 * LJ_A, -LJ_A, 3 * LJ_A), 7),  # tilts of whole lattice spacings: the lattice stays periodic
    "hex": ((LJ_L, LJ_L, LJ_L, 2 * LJ_A, 0.0, 0.0), 3),
}


def lj_band_particles(q, box6, mask, cuts, rel, pairs=None, rows=None):
    """Particles (of rows) with a partner whose r^2 is within rel (relative) of some cut^2: where a rounding of the
    position type could decide the cut-off test the other way."""
    I, J, d, _ = lj_pairs(q, box6, mask, max(cuts) * (1 + rel), rows=rows) if pairs is None else pairs
    r2 = np.sort(np.einsum("ij,ij->i", d, d))
    order = np.argsort(np.einsum("ij,ij->i", d, d))
    bad = np.zeros(len(r2), dtype=bool)
    for c in cuts:
        lo, hi = np.searchsorted(r2, [c * c * (1 - rel), c * c * (1 + rel)])
        bad[order[lo:hi]] = True
    return np.unique(I[bad])


def lj_fractional(p, box6):
    """Coordinates of p[k, 3] along the edge vectors a, b, c of the box (LAMMPS convention), in [0, 1) inside the cell."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box6)
    lz = p[:, 2] / Lz
    ly = (p[:, 1] - lz * yz) / Ly
    lx = (p[:, 0] - ly * xy - lz * xz) / Lx
    return np.stack([lx, ly, lz], axis=1)


def lj_lattice_vectors(k, box6, mask):
    """k_a a + k_b b + k_c c for k[n, 3], the components of the open axes of mask taken as 0."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box6)
    k = np.asarray(k, dtype=np.float64) * [mask & 1, mask >> 1 & 1, mask >> 2 & 1]
    return np.stack([k[:, 0] * Lx + k[:, 1] * xy + k[:, 2] * xz, k[:, 1] * Ly + k[:, 2] * yz, k[:, 2] * Lz], axis=1)


def lj_lattice(seed, box="xyz", cuts=(2.5,)):
    """n = 2744 positions [n, 4], float32 values held in float64: sites (k + 1/2) a of the 14^3 lattice jittered by
    +-0.10 per axis (closest pair 0.925), so every coordinate is inside [0, L).  Particles with a partner within 2^-15
    (relative, r^2) of a cut-off of `cuts` get their jitter drawn again: no cut-off test hangs on a rounding."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(LJ_M),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    site = (g + 0.5) * LJ_A
    q = np.zeros((len(g), 4))
    box6, mask = LJ_BOXES[box]

    def place(p):  # into the (tilted) cell on the periodic axes, by whole lattice vectors; then float32 values
        return lj_wrap(p, box6, mask).astype(np.float32)

    q[:, :3] = place(site + rng.uniform(-0.1, 0.1, size=site.shape))
    bad = None
    for _ in range(20):  # (a pair that enters the band has a particle drawn again: only those need another look)
        bad = lj_band_particles(q, box6, mask, cuts, 2.0 ** -15, rows=bad)
        if not len(bad):
            return q
        q[bad, :3] = place(site[bad] + rng.uniform(-0.1, 0.1, size=(len(bad), 3)))
    raise AssertionError("lj_lattice: pairs stay in the cut-off band")


def lj_wrap(p, box6, mask):
    """p[k, 3] moved into the cell on the periodic axes by whole lattice vectors (float64)."""
    return p + lj_lattice_vectors(-np.floor(lj_fractional(p, box6)), box6, mask)


def lj_drift(q, seed, box="xyz", k=None):
    """Adds to every particle a whole lattice vector k_a a + k_b b + k_c c, k drawn from {-1, 0, +1} on each periodic
    axis: positions that have drifted and were never wrapped.  Every coordinate along the edge vectors stays within one
    box length of the cell (a particle within 2^-10 of a face keeps k = 0 on that axis, so that no rounding puts it past
    the limit).  box: a name of LJ_BOXES or (box6, mask).  Returns float64; the caller rounds to its position type."""
    box6, mask = LJ_BOXES[box] if isinstance(box, str) else box
    rng = np.random.default_rng(seed)
    k = rng.integers(-1, 2, size=(len(q), 3)).astype(np.float64) if k is None else np.array(k, dtype=np.float64)
    l = lj_fractional(q[:, :3], box6)
    k[(l < 2.0 ** -10) | (l > 1 - 2.0 ** -10)] = 0
    out = q.copy()
    out[:, :3] = q[:, :3] + lj_lattice_vectors(k, box6, mask)
    return out


def lj_type_params(nt, rc_list, seed=7):
    """(types[n], rc_ab, eps_ab, sig_ab, rcf_ab) of the typed cases, nt x nt symmetric: eps_ab = sqrt(e_a e_b) with e spanning
    a factor 50 (0.2 .. 10), sig_ab = (s_a + s_b) / 2 from 0.9 to 1.1, rc_force_ab = 2.5 sig_ab / 1.1 (a cut-off per sigma,
    at most 2.5), list cut-offs rc_ab = rc_list -- except rc_ab = rc_force_ab = 0 for the pair (0, nt - 1), whose entries
    leave the list.  Types are dealt evenly, so every type occurs as row type and as partner type."""
    rng = np.random.default_rng(seed)
    n = LJ_M ** 3
    types = rng.permutation(np.arange(n) % nt).astype(np.int32)
    e = 0.2 * 50.0 ** (rng.permutation(nt) / max(nt - 1, 1))
    s = 0.9 + 0.2 * rng.permutation(nt) / max(nt - 1, 1)
    eps = np.sqrt(e[:, None] * e[None, :])
    sig = 0.5 * (s[:, None] + s[None, :])
    rcf = 2.5 * sig / 1.1
    rc = np.full((nt, nt), float(rc_list))
    rc[0, nt - 1] = rc[nt - 1, 0] = rcf[0, nt - 1] = rcf[nt - 1, 0] = 0.0
    return types, rc, eps, sig, rcf


def lj_pair_magnitudes(n, rows, cols, d, r2, eps=1.0, sig=1.0, inn=None):
    """S of lj_reference from the pair arrays of a half list (every pair once; d, r2 at the image; inn: pairs within
    rc_force): for the comparisons that sum over a list."""
    s6 = (sig * sig / r2) ** 3
    s12 = s6 * s6
    fa, ua = 24.0 * np.abs(eps) * (2.0 * s12 + s6) / r2, 2.0 * np.abs(eps) * (s12 + s6)
    if inn is not None:
        fa, ua = np.where(inn, fa, 0.0), np.where(inn, ua, 0.0)
    S = np.zeros((n, 4))
    for c in range(3):
        w = fa * np.abs(d[:, c])
        S[:, c] = np.bincount(rows, weights=w, minlength=n) + np.bincount(cols, weights=w, minlength=n)
    S[:, 3] = np.bincount(rows, weights=ua, minlength=n) + np.bincount(cols, weights=ua, minlength=n)
    return S


def lj_rows_off_the_band(n, rows, cols, r2, rcf, dtype):
    """Particles without a partner within 64 ulp (of the position type, in r) of rc_force: where the cut-off test is exact."""
    band = np.abs(r2 / (rcf * rcf) - 1.0) < 2 * 64 * lj_unit(dtype)
    ok = np.ones(n, dtype=bool)
    ok[rows[band]] = False
    ok[cols[band]] = False
    return ok

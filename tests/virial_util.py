"""What tests/test_lj_virial.py checks nl_lj_virial against: an O(N^2) float64 reference, a numpy emulation of the kernel's
arithmetic in the position type, and the bound |got - want| <= VIR_C u S per component."""
import numpy as np

from tests.util import _lj_par, emulate_pairs, lj_pairs, lj_unit  # noqa: F401 (emulate_pairs: for the importers of this module)

# 4 x the largest per-row ratio of test_emulation_gives_c (virial_emulate over EMULATED, both list kinds, three orders)
VIR_C = 47.6
COLS = ("xx", "yy", "zz", "xy", "xz", "yz", "U", "n_in")
_AB = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _row_sums(n, I, cols):
    out = np.zeros((n, len(cols)))
    for c, w in enumerate(cols):
        out[:, c] = np.bincount(I, weights=w, minlength=n)
    return out


def virial_rows(n, I, d, e, s):
    """Per row i, over the ordered pairs (I, .) given (already within the cut-off, separations d at the image): the float64
    sums (row[n, 7], S_row[n, 7]) of d_a F_b for the six components and of the pair's full energy, with their uncancelled
    magnitudes 24 |eps| (2 s12 + s6) / r^2 |d_a d_b| and 4 |eps| (s12 + s6)."""
    r2 = (d * d).sum(axis=1)
    s6 = (s * s / r2) ** 3
    s12 = s6 * s6
    fr = 24.0 * e * (2.0 * s12 - s6) / r2
    fa = 24.0 * np.abs(e) * (2.0 * s12 + s6) / r2
    row = _row_sums(n, I, [fr * d[:, a] * d[:, b] for a, b in _AB] + [4.0 * e * (s12 - s6)])
    S = _row_sums(n, I, [fa * np.abs(d[:, a] * d[:, b]) for a, b in _AB] + [4.0 * np.abs(e) * (s12 + s6)])
    return row, S


def virial_reference(q, box6, mask, eps, sig, rcf, types=None, exclusions=None, pairs=None):
    """W_ab = sum over pairs d_a F_b, U and the number of pairs with 0 < r^2 < rcf_ab^2 by an O(N^2) float64 sum that uses
    no list: (want[8] = {W_xx, W_yy, W_zz, W_xy, W_xz, W_yz, U, n_in}, S[7], rows).  d = r_i - r_j, F the force on i
    (tests.util lj_reference's): every unordered pair once.  rows: what the emulation test needs, per list kind the
    ordered pairs (I, J) a list of that kind holds (full: both orders; half: i < j) and their per-row (sums, S)."""
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
    I, J, d = I[keep], J[keep], d[keep]
    e, s = (np.broadcast_to(v, keep.shape)[keep] for v in (e, s))
    rows = {}
    for kind, sel in (("full", np.ones(len(I), dtype=bool)), ("half", I < J)):
        rows[kind] = (I[sel], J[sel]) + virial_rows(n, I[sel], d[sel], e[sel], s[sel])
    row, S_row = rows["full"][2:]
    want = np.concatenate([0.5 * row.sum(axis=0), [0.5 * len(I)]])
    assert len(I) % 2 == 0
    return want, 0.5 * S_row.sum(axis=0), rows


def virial_ratio(got, want, S, dtype):
    """|got - want| / (u S) for the 7 sums (inf where got is not finite, or differs where the bound vanishes)."""
    got = np.asarray(got, dtype=np.float64)
    err, den = np.abs(got[..., :7] - want[..., :7]), lj_unit(dtype) * np.asarray(S)[..., :7]
    r = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(r), r, np.inf)


def check_virial(got, want, S, dtype, c=VIR_C, count=True):
    """Asserts |got - want| <= c u S for each of the 7 sums and, with count, n_in exactly."""
    r = virial_ratio(got, want, S, dtype)
    k = int(np.argmax(r))
    assert r[k] <= c, f"{COLS[k]}: |got - want| = {r[k]:.4g} u S, allowed {c:g} (all: {np.round(r, 3)}; got {got}, want {want})"
    if count:
        assert got[7] == want[7], f"n_in: got {got[7]}, want {want[7]}"


def virial_emulate(n, I, vals, rng):
    """The row body of k_lj_virial over emulate_pairs' values: the six products and the energy in T, one rounding each,
    converted to double and added in double, every row's entries in a random order (the kernel deals them to 64 lanes
    and adds the lanes in a butterfly).  Returns (rows[n, 7] in float64, n_in)."""
    dx, dy, dz, fx, fy, fz, pe, inn = vals
    terms = [fx * dx, fy * dy, fz * dz, fx * dy, fx * dz, fy * dz, pe]
    assert all(t.dtype == dx.dtype for t in terms)
    order = np.lexsort((rng.random(len(I)), I))
    rows = _row_sums(n, I[order], [t.astype(np.float64)[order] for t in terms])  # (bincount adds in the order given)
    return rows, int(inn.sum())

"""The Steinhardt family's reference, error model, emulation and checker (tests/test_steinhardt.py).

reference()   an O(N^2) evaluation over lj_pairs that uses no list, in long double and rounded to float64 once: Y_lm from Legendre
              polynomials (the m-th derivative of P_l as a Legendre series, Clenshaw's sum) and arctan2, independent of the
              recurrence the kernels use and equal to scipy's harmonics to 1e-13; with every value a scale S, a first-order
              propagation of the roundings of the rule of nl_set_steinhardt (include/nl_hip.h).
emulate()     the rule itself in numpy in the position type T, one rounding per operation, random summation orders; `defect`
              breaks it in one of DEFECTS' ways.
ratios()      |got - want| / (u S) per family of values; check() asserts them within STEIN_C and N_b exact.

The scales.  u is the unit roundoff of T, Ymax = sqrt((2 l + 1) / (4 pi)) bounds every |Y_lm|.
  q_lm   a bond's unit vector carries a few u (the separation, r2, sqrt, division, product), and |grad Y_lm| <= sqrt(l (l + 1))
         Ymax; the degree recurrence and the complex power add l roundings of terms of that size; the sum over N_b bonds is
         ceil(N_b / 64) adds per lane and 6 across the wave.  So  S_qlm = Ymax (l + 1 + 6 + ceil(N_b / 64)),  for re and im alike.
  s      = sum_m w_m |q_lm|^2, w_0 = 1, w_m = 2:  S_s = 2 sum_m w_m (|re| + |im|) S_qlm + 6 s.
  q_l    = sqrt(c s):  S_q = c S_s / (2 q_l) + 2 q_l.
  W      = sum W[m1][m2] Re(q_m1 q_m2 q_m3):  S_W = sqrt(2) S_qlm sum |W| (a1 a2 + a2 a3 + a1 a3) + (14 + ceil(nterms / 64)) sum |W| a1 a2 a3,
         a = |q_lm|.
  w_l    = W / s^(3/2):  S_w = S_W / s^(3/2) + (3/2) |w_l| S_s / s + 3 |w_l|.
  averaged q_lm = (q_lm(i) + sum_k q_lm(k)) / (N_b + 1):  S = (S_qlm(i) + sum_k S_qlm(k)) / (N_b + 1) + (8 + ceil(N_b / 64)) (|q(i)| +
         sum_k |q(k)|) / (N_b + 1) per part; the averaged q_l and w_l from it by the same formulas.
STEIN_C is 4 x the largest ratio the float32 emulation reaches on the lattice and dimer inputs (test_emulation_gives_c recomputes
it), the 4 for the device's other order of summation and of the walk.
"""
import functools

import numpy as np
from scipy import special

from md_neighbor_list_amd import steinhardt as st
from tests.util import lj_list_separations, lj_pairs, lj_unit

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"

# 4 x the emulation's largest ratios (float32, the parity inputs): q_lm; q_l and its averaged form; w_l and its averaged form.
# Emulated: 5.275, 1.920, 0.0533 (test_emulation_gives_c).  The device reaches, fp32 / fp64, over the GPU tests: 5.275 / 4.077,
# 1.920 / 1.536, 0.104 / 0.064 (a dimer's fp32 figures repeat the emulation: one bond, the same operations); DESIGN.md section 8z.
# The largest are a lone bond's at l = 12 (the isolated dimers): the errors of the one bond's Y_lm are those of one z and one
# recurrence, and nothing averages them.  A first set of inputs held the lattices alone (N_b >= 3), whose emulation gives 0.884 and
# 0.240; the emulation of the dimers showed that the rule itself exceeds 4 x that there, and the dimers joined the set.
STEIN_C = {"qlm": 21.2, "q": 7.7, "w": 0.22}
# The reference's own error, in units of 2^-53 S: it works in long double and its results are rounded to double once, which is
# nothing beside a float32 result and a little beside a float64 one (with harmonics in double -- lpmv, exp(i m phi) -- it was 15 of
# these units, more than the rule's own error).  2 x the largest ratio of the reference against the rule evaluated in long double
# (tables included), the 2 for inputs other than the measured ones.  Measured: 0.098, 0.040, 0.0054 (test_reference_error).
REF_C = {"qlm": 0.2, "q": 0.082, "w": 0.011}

DEFECTS = ("a dropped neighbour", "r_i - r_j for r_j - r_i", "no self term in the average", "/ N_b for / (N_b + 1)",
           "no factor 2 on m > 0", "w_l not normalised")


def ymax(l):
    return np.sqrt((2 * l + 1) / (4 * np.pi))


def ylm(l, x, y, z):
    """Y_lm of unit vectors for m = 0 .. l, (k, l + 1) complex, Condon-Shortley phase (scipy's sph_harm convention): from
    Legendre polynomials (numpy.polynomial.legendre: the m-th derivative of P_l as a Legendre series, Clenshaw's sum) and arctan2,
    in long double, so that the reference's own error is small beside a float64 result too."""
    from math import factorial

    from numpy.polynomial import legendre

    x, y, z = (np.asarray(v, dtype=LD) for v in (x, y, z))
    phi, s = np.arctan2(y, x), np.sqrt(x * x + y * y)
    pi = 4 * np.arctan(LD(1))
    out = np.zeros((len(z), l + 1), dtype=np.clongdouble)
    for m in range(l + 1):
        # P_l^m = (-1)^m (1 - z^2)^(m/2) d^m P_l / dz^m, the derivative as a Legendre series (small integers: exact)
        val = legendre.legval(z, legendre.legder([0.0] * l + [1.0], m).astype(LD)) * s ** m * (-1) ** m
        norm = np.sqrt(LD(2 * l + 1) / (4 * pi) * LD(factorial(l - m)) / LD(factorial(l + m)))
        out[:, m] = norm * val * (np.cos(m * phi) + 1j * np.sin(m * phi))
    return out


def row_sum(I, vals, n):
    """out[i] = sum of vals[k] over I[k] == i, in the type of vals (long double stays long double)."""
    out = np.zeros((n,) + vals.shape[1:], dtype=vals.dtype)
    if len(I):
        order = np.argsort(I, kind="stable")
        Is = I[order]
        starts = np.flatnonzero(np.r_[True, Is[1:] != Is[:-1]])
        out[Is[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def scipy_ylm(l, m, x, y, z):
    """scipy's own harmonics at unit vectors, whichever name this scipy has."""
    theta, phi = np.arccos(np.clip(z, -1.0, 1.0)), np.arctan2(y, x)  # polar, azimuth
    if hasattr(special, "sph_harm_y"):
        return special.sph_harm_y(l, m, theta, phi)
    return special.sph_harm(m, l, phi, theta)


def full_qlm(q):
    """(n, l + 1) of m = 0 .. l to (n, 2 l + 1) of m = -l .. l by q_{l,-m} = (-1)^m conj(q_lm)."""
    l = q.shape[1] - 1
    m = np.arange(1, l + 1)
    return np.concatenate([(np.conj(q[:, 1:]) * (-1.0) ** m)[:, ::-1], q], axis=1)


@functools.lru_cache(maxsize=None)
def w3j_terms(l):
    """The non-zero terms (i1, i2, i3, W) of the 3j table, indices m + l."""
    w = st.wigner3j_table(l)
    i1, i2 = np.nonzero(w)
    return i1, i2, 3 * l - i1 - i2, w[i1, i2]


def neighbours(q, box6, mask, r_max, types=None, rc_ab=None, exclusions=None, pairs=None):
    """(I, J, d = r_i - r_j) of the neighbour pairs, both orders: 0 < r < r_max, not excluded, not of a type pair with
    rc_ab = 0.  d to float64 accuracy of the folded separation (lj_list_separations)."""
    n = len(q)
    I, J, d, _ = lj_pairs(q, box6, mask, r_max) if pairs is None else pairs
    r2 = (d * d).sum(axis=1)
    keep = (r2 > 0) & (r2 < r_max * r_max)
    if types is not None and rc_ab is not None:
        t = np.asarray(types, dtype=np.int64)
        keep &= np.asarray(rc_ab)[t[I], t[J]] > 0
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keep &= ~np.isin(I * n + J, np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]]))
    I, J = I[keep], J[keep]
    return I, J, lj_list_separations(q, I, J, box6, mask)


def _columns(qf, Sq, l):
    """(q_l, w_l, S_q, S_w) from q_lm of m = -l .. l (n, 2 l + 1) and the scale Sq (n,) of its parts."""
    a = np.abs(qf)
    s = (a * a).sum(axis=1)
    wm = np.where(np.arange(-l, l + 1) == 0, 1.0, 2.0)[l:]
    half = qf[:, l:]
    Ss = 2.0 * (wm * (np.abs(half.real) + np.abs(half.imag))).sum(axis=1) * Sq + 6.0 * s
    c = 4 * np.pi / (2 * l + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ql = np.sqrt(c * s)
        S_q = c * Ss / (2 * ql) + 2 * ql
        i1, i2, i3, W = w3j_terms(l)
        prod = qf[:, i1] * qf[:, i2] * qf[:, i3]
        Wsum = (W * prod.real).sum(axis=1)
        a1, a2, a3 = a[:, i1], a[:, i2], a[:, i3]
        S_W = np.sqrt(2.0) * Sq * (np.abs(W) * (a1 * a2 + a2 * a3 + a1 * a3)).sum(axis=1)
        S_W += (14 + -(-len(W) // 64)) * (np.abs(W) * a1 * a2 * a3).sum(axis=1)
        wl = Wsum / s ** 1.5
        S_w = S_W / s ** 1.5 + 1.5 * np.abs(wl) * Ss / s + 3 * np.abs(wl)
    return ql, wl, S_q, S_w


def reference(q, box6, mask, l, r_max, types=None, rc_ab=None, exclusions=None, pairs=None):
    """The order parameters of every particle in float64: a dict of
       nb (n,) int, qlm (n, l + 1) complex, S_qlm (n,), cols (n, 4) = {q_l, w_l, averaged q_l, averaged w_l}, S (n, 4).
    N_b = 0: NaN in qlm and cols."""
    n = len(q)
    I, J, d = neighbours(q, box6, mask, r_max, types, rc_ab, exclusions, pairs)
    dl = d.astype(LD)
    u = -dl / np.sqrt((dl * dl).sum(axis=1))[:, None]
    Y = ylm(l, u[:, 0], u[:, 1], u[:, 2])
    nb = np.bincount(I, minlength=n)
    with np.errstate(invalid="ignore", divide="ignore"):  # (everything in long double; rounded to double at the end)
        qlm = row_sum(I, Y, n) / nb.astype(LD)[:, None]
        Sq = np.where(nb > 0, ymax(l) * (l + 1 + 6 + -(-nb // 64)), np.nan)
        ql, wl, S_q, S_w = _columns(full_qlm(qlm), Sq, l)
        # the average over the same neighbours
        tot = qlm + row_sum(I, qlm[J], n)
        mag = np.maximum(np.abs(qlm.real), np.abs(qlm.imag))
        mag = (mag + row_sum(I, mag[J], n)).max(axis=1).astype(np.float64)
        Sa = (Sq + np.bincount(I, weights=Sq[J], minlength=n)) / (nb + 1)
        Sa = Sa + (8 + -(-nb // 64)) * mag / (nb + 1)
        qa = tot / (nb + 1).astype(LD)[:, None]
        qal, wal, S_qa, S_wa = _columns(full_qlm(qa), Sa, l)
    f64 = lambda *a: np.stack([np.asarray(v, dtype=np.float64) for v in a], axis=1)  # noqa: E731
    return {"nb": nb, "qlm": qlm.astype(np.complex128), "S_qlm": Sq, "cols": f64(ql, wl, qal, wal), "S": f64(S_q, S_w, S_qa, S_wa),
            "qa": qa.astype(np.complex128), "S_qa": Sa, "pairs": (I, J, d)}


# ------------------------------------------------------------------------------------------------------ the emulation
def tables(l, T):
    """{A_km, B_km} (k > m), S_m (at k = m) and c = 4 pi / (2 l + 1), formed in double and rounded to T once (nl_set_steinhardt)."""
    D = np.longdouble if T == np.longdouble else np.float64  # (long double: the tables of test_reference_error's yardstick)
    pi = 4 * np.arctan(D(1))
    A, B = np.zeros((l + 1, l + 1), dtype=D), np.zeros((l + 1, l + 1), dtype=D)
    for m in range(l + 1):
        pr = D(1)
        for i in range(1, m + 1):
            pr *= D(2 * i - 1) / D(2 * i)
        A[m, m] = (-1) ** m * np.sqrt(D(2 * m + 1) / (4 * pi) * pr)
        for k in range(m + 1, l + 1):
            A[m, k] = np.sqrt(D(4 * k * k - 1) / D(k * k - m * m))
            B[m, k] = A[m, k] * np.sqrt(D((k - 1) ** 2 - m * m) / D(4 * (k - 1) ** 2 - 1))
    return A.astype(T), B.astype(T), T(4 * pi / D(2 * l + 1))


def _ordered_sum(I, terms, n, T, rng):
    """sum of terms[k] into row I[k], in T, one rounding per add, in a random order per row.  terms: (k, c)."""
    out = np.zeros((n, terms.shape[1]), dtype=T)
    order = rng.permutation(len(I))
    order = order[np.argsort(I[order], kind="stable")]
    Is = I[order]
    first = np.searchsorted(Is, Is)
    rank = np.arange(len(Is)) - first
    ts = terms[order]
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        out[Is[sel]] += ts[sel]
    return out


def _emulated_columns(re, im, l, T, rng, W, defect):
    """{q_l, w_l} by the rule from q_lm of m = 0 .. l in T (re, im: (n, l + 1))."""
    n = len(re)
    A, B, c = tables(l, T)
    v = re * re + im * im
    terms = np.concatenate([v[:, :1], v[:, 1:] if defect == "no factor 2 on m > 0" else v[:, 1:] + v[:, 1:]], axis=1)
    s = np.zeros(n, dtype=T)
    for m in rng.permutation(l + 1):
        s = s + terms[:, m]
    with np.errstate(invalid="ignore", divide="ignore"):
        ql = np.sqrt(c * s)
        if W is None:
            return ql, np.full(n, np.nan, dtype=T)
        sg = np.where(np.arange(1, l + 1) % 2 == 1, T(-1), T(1)).astype(T)
        fr = np.concatenate([(sg * re[:, 1:])[:, ::-1], re], axis=1)
        fi = np.concatenate([(-(sg * im[:, 1:]))[:, ::-1], im], axis=1)
        i1, i2, i3, Wv = w3j_terms(l)
        Wv = Wv.astype(T)
        acc = np.zeros(n, dtype=T)
        for t in rng.permutation(len(Wv)):
            a, b, cc = i1[t], i2[t], i3[t]
            pr = fr[:, a] * fr[:, b] - fi[:, a] * fi[:, b]
            pi = fr[:, a] * fi[:, b] + fi[:, a] * fr[:, b]
            acc = acc + Wv[t] * (pr * fr[:, cc] - pi * fi[:, cc])
        wl = acc if defect == "w_l not normalised" else acc / (s * np.sqrt(s))
    return ql, wl


def emulate(q, l, T, rng, nbrs, w=True, defect=None):
    """The rule of nl_set_steinhardt in T over the neighbour pairs nbrs = (I, J, d) of neighbours(): a dict of nb, qlm (complex128
    holding T values) and cols (n, 4) in T."""
    n = len(q)
    I, J, d = nbrs
    if defect == "a dropped neighbour":  # (the first neighbour of every third centre)
        first = np.unique(I, return_index=True)[1]
        keep = np.ones(len(I), dtype=bool)
        keep[first[::3]] = False
        I, J, d = I[keep], J[keep], d[keep]
    d = d.astype(T)
    if defect == "r_i - r_j for r_j - r_i":
        d = -d
    A, B, c = tables(l, T)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    r2 = (dx * dx + dy * dy) + dz * dz
    ir = T(1) / np.sqrt(r2)
    x, y, z = (-dx) * ir, (-dy) * ir, (-dz) * ir
    cr, ci = np.ones(len(I), dtype=T), np.zeros(len(I), dtype=T)
    Yr, Yi = np.zeros((len(I), l + 1), dtype=T), np.zeros((len(I), l + 1), dtype=T)
    for m in range(l + 1):
        if m > 0:
            cr, ci = cr * x - ci * y, cr * y + ci * x
        p1, p2 = np.full(len(I), A[m, m], dtype=T), np.zeros(len(I), dtype=T)
        for k in range(m + 1, l + 1):
            p1, p2 = (A[m, k] * z) * p1 - B[m, k] * p2, p1
        Yr[:, m], Yi[:, m] = p1 * cr, p1 * ci
    nb = np.bincount(I, minlength=n)
    sums = _ordered_sum(I, np.concatenate([Yr, Yi], axis=1), n, T, rng)
    with np.errstate(invalid="ignore", divide="ignore"):
        fn = nb.astype(T)[:, None]
        re, im = sums[:, :l + 1] / fn, sums[:, l + 1:] / fn
        W = st.wigner3j_table(l) if w else None
        ql, wl = _emulated_columns(re, im, l, T, rng, W, defect)
        gath = _ordered_sum(I, np.concatenate([re[J], im[J]], axis=1), n, T, rng)
        den = (nb if defect == "/ N_b for / (N_b + 1)" else nb + 1).astype(T)[:, None]
        if defect == "no self term in the average":
            ar, ai = gath[:, :l + 1] / den, gath[:, l + 1:] / den
        else:
            ar, ai = (re + gath[:, :l + 1]) / den, (im + gath[:, l + 1:]) / den
        qal, wal = _emulated_columns(ar, ai, l, T, rng, W, defect)
    return {"nb": nb, "qlm": re.astype(np.float64) + 1j * im.astype(np.float64), "cols": np.stack([ql, wl, qal, wal], axis=1),
            "qa": ar.astype(np.float64) + 1j * ai.astype(np.float64)}


# -------------------------------------------------------------------------------------------------------- the checker
def _ratio(got, want, S, dtype):
    """|got - want| / (u S); 0 where both are NaN (a centre without neighbours), inf where only one is."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / (lj_unit(dtype) * S)
    r = np.where(np.isnan(r), np.inf, r)
    return np.where(both, 0.0, np.where(np.abs(got - want) == 0, 0.0, r))


def ratios(got, ref, dtype, average=True, w=True, rows=None):
    """The largest |got - want| / (u S) of {"qlm", "q", "w"} over every particle (of rows); got: a dict of nb, qlm, cols as
    emulate() returns it (the device's: test_steinhardt.device_result)."""
    rows = slice(None) if rows is None else rows
    rq = np.maximum(_ratio(got["qlm"].real, ref["qlm"].real, ref["S_qlm"][:, None], dtype),
                    _ratio(got["qlm"].imag, ref["qlm"].imag, ref["S_qlm"][:, None], dtype))[rows]
    rc = _ratio(got["cols"], ref["cols"], ref["S"], dtype)[rows]
    qcols, wcols = ([0, 2], [1, 3]) if average else ([0], [1])
    out = {"qlm": float(rq.max(initial=0.0)), "q": float(rc[:, qcols].max(initial=0.0))}
    if w:
        out["w"] = float(rc[:, wcols].max(initial=0.0))
    return out


def check(got, ref, dtype, average=True, w=True, rows=None, c=None):
    """Asserts N_b exact and every value within c u S, family by family; returns the ratios."""
    c = STEIN_C if c is None else c
    assert np.array_equal(np.asarray(got["nb"]), ref["nb"]), "N_b differs"
    r = ratios(got, ref, dtype, average, w, rows)
    for k, v in r.items():
        lim = c[k] + REF_C[k] * 2.0 ** -53 / lj_unit(dtype)  # (the reference's own error: nothing in float32, REF_C in float64)
        assert v <= lim, f"{k}: {v:.3g} u S > {lim:.3g} u S"
    return r


# ------------------------------------------------------------------------------------------------------------ crystals
def crystal(name, cells, a=1.6):
    """(q (n, 4) float64, box6, r_max_1, r_max_2): a perfect periodic lattice of cubic (hcp: orthorhombic) cells of edge a, and
    neighbour ranges between its first and second, and second and third shell.  Every coordinate is a float32 value where a
    is (hcp: rounded to float32, so that its shell is ideal only to that rounding -- the reference sees the same positions)."""
    if name == "hcp":
        c = a * np.sqrt(8.0 / 3.0)
        cell = np.array([a, a * np.sqrt(3.0), c])
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 5.0 / 6.0, 0.5], [0, 1.0 / 3.0, 0.5]])
        shells = (a, a * np.sqrt(2.0))
    else:
        cell = np.array([a, a, a])
        basis = {"sc": [[0, 0, 0]], "bcc": [[0, 0, 0], [0.5, 0.5, 0.5]],
                 "fcc": [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]}[name]
        basis = np.array(basis, dtype=np.float64)
        shells = {"sc": (a, a * np.sqrt(2.0), a * np.sqrt(3.0)), "bcc": (a * np.sqrt(0.75), a, a * np.sqrt(2.0)),
                  "fcc": (a * np.sqrt(0.5), a, a * np.sqrt(1.5))}[name]
    g = np.stack(np.meshgrid(*(np.arange(cells),) * 3, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    p = ((g + basis[None, :, :]) * cell).reshape(-1, 3)
    box = (cells * cell).astype(np.float32).astype(np.float64)
    q = np.zeros((len(p), 4))
    q[:, :3] = p.astype(np.float32)
    r1 = 0.5 * (shells[0] + shells[1])
    r2 = 0.5 * (shells[1] + shells[2]) if len(shells) > 2 else None
    return q, (box[0], box[1], box[2], 0.0, 0.0, 0.0), r1, r2

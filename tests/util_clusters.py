"""References, the solid-bond band, the emulation and the checkers of nl_clusters and nl_solid_bonds (tests/test_clusters.py,
DESIGN.md section 8za).  Nothing here reads a list, the library's or the oracle's.

Clusters.  edges() takes the O(N^2) float64 minimum-image pair search of tests.util (lj_pairs), reference() hands the pairs
within r_max between members to scipy.sparse.csgraph.connected_components and canonicalises the answer to the smallest particle
index of every component.  check() demands labels, sizes and summary equal to it, element for element.

Solid bonds.  solid_reference() evaluates the rule of nl_solid_bonds (include/nl_hip.h) in float64 on the float64 q_lm of
tests.util_steinhardt.reference: per ordered neighbour pair the margin  M_ij = D_ij - thr sqrt(s_i s_j)  and a scale S_ij, a
first-order propagation of everything that separates a result in T from it (u the unit roundoff of T):
  q_lm     both ends carry STEIN_C["qlm"] u S_qlm per part (the tested bound of section 8z).  Through the bilinear form,
           with w_0 = 1, w_m = 2 and a_m(i) = |re_im| + |im_im|:   A_ij = sum_m w_m (a_m(j) S_qlm(i) + a_m(i) S_qlm(j));
           through the right-hand side, s_i moving by A_ii = 2 sum_m w_m a_m(i) S_qlm(i):
           R_ij = |thr| (s_j A_ii + s_i A_jj) / (2 sqrt(s_i s_j)).
  the form 2 l + 4 roundings on the sum of the magnitudes of its terms, T_ij = sum_m w_m (|re_im re_jm| + |im_im im_jm|), and the
           same for s_i = T_ii and s_j through the right-hand side.
  rhs      the product s_i s_j, the square root and the product with thr: 3 |thr| sqrt(s_i s_j).
  S_ij = STEIN_C["qlm"] (A_ij + R_ij) + (2 l + 4) (T_ij + |thr| (s_j T_ii + s_i T_jj) / (2 sqrt(s_i s_j))) + 3 |thr| sqrt(s_i s_j).
A bond is "sure" where M_ij > SOLID_C u S_ij, "banded" where |M_ij| <= SOLID_C u S_ij: a device may decide a banded bond either
way.  SOLID_C is 4 x the largest |M_ij(T) - M_ij| / (u S_ij) of a float32 numpy emulation of the rule (solid_emulate, one rounding
per operation, on the q_lm of util_steinhardt.emulate) over the inputs of tests/test_clusters.py, the dimers included;
test_emulation_gives_solid_c recomputes it.  It comes from the emulation and the reference, never from a device.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import util_steinhardt as us
from tests.util import lj_unit

# 4 x the emulation's largest ratio (float32): 0.0123 on the inputs of test_emulation_gives_solid_c (the dimers give it; the
# lattices, the half-crystal box and the liquid reach 0.002 to 0.003).  The scale is dominated by the tested q_lm bound, STEIN_C u
# S_qlm, which an actual q_lm stays far inside, so the constant is small.  The device reaches on the half-crystal box, fp32 / fp64:
# 0.0029 / 0.0023.
SOLID_C = 0.05

CLUSTER_DEFECTS = ("a dropped edge", "a label that is not the minimum", "a non-member united through", "a member left at -1",
                   "sizes off by the root's own count", "a tie broken towards the larger label")


# ------------------------------------------------------------------------------------------------------------ clusters
def edges(pairs, r_max, n, exclusions=None):
    """(I, J) with I < J: the unordered pairs of lj_pairs' result within r_max, less the excluded ones."""
    I, J, d, _ = pairs
    r2 = np.einsum("ij,ij->i", d, d)
    keep = (r2 < r_max * r_max) & (I < J)
    I, J = I[keep], J[keep]
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        lo, hi = ex.min(axis=1), ex.max(axis=1)
        keep = ~np.isin(I * n + J, lo * n + hi)
        I, J = I[keep], J[keep]
    return I, J


def summary_of(labels, sizes):
    """{members, clusters, size of the largest cluster, its label} from canonical labels; ties to the smallest label."""
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    if not len(roots):
        return np.array([0, 0, 0, -1], dtype=np.int64)
    best = roots[np.argmax(sizes[roots])]  # (argmax takes the first of equals, roots ascend)
    return np.array([(labels >= 0).sum(), len(roots), sizes[best], best], dtype=np.int64)


def reference(n, I, J, member=None, defect=None):
    """(labels, sizes, summary) of the graph on n particles with the edges (I, J) between members (member: bool (n,) or None),
    by scipy's connected_components, canonicalised: a member's label is the smallest index of its component, a non-member's
    -1; sizes 0 for a non-member.  defect: one of CLUSTER_DEFECTS, for the checker's own test."""
    mem = np.ones(n, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    use = np.ones(len(I), dtype=bool) if defect == "a non-member united through" else mem[I] & mem[J]
    I, J = I[use], J[use]
    if defect == "a dropped edge" and len(I):  # (every edge of one particle that has some: it becomes a singleton)
        v = I[len(I) // 2]
        keep = (I != v) & (J != v)
        I, J = I[keep], J[keep]
    comp = connected_components(coo_matrix((np.ones(len(I), dtype=np.int8), (I, J)), shape=(n, n)), directed=False)[1]
    comp = np.where(mem, comp, -1)
    labels = np.full(n, -1, dtype=np.int64)
    idx = np.flatnonzero(mem)
    if len(idx):
        first = np.full(comp.max() + 1, n, dtype=np.int64)
        np.minimum.at(first, comp[idx], idx)
        if defect == "a label that is not the minimum":
            first = np.full(comp.max() + 1, -1, dtype=np.int64)
            np.maximum.at(first, comp[idx], idx)
        labels[idx] = first[comp[idx]]
    if defect == "a member left at -1" and len(idx):
        labels[idx[len(idx) // 3]] = -1
    sizes = np.zeros(n, dtype=np.int64)
    m = labels >= 0
    sizes[m] = np.bincount(labels[m], minlength=n)[labels[m]]
    if defect == "sizes off by the root's own count":
        sizes[m] -= 1
    summary = summary_of(labels, sizes)
    if defect == "a tie broken towards the larger label":
        roots = np.flatnonzero(labels == np.arange(n))
        top = roots[sizes[roots] == sizes[roots].max()]
        assert len(top) > 1, "the input has no tie for the largest cluster"
        summary[3] = top[-1]
    return labels.astype(np.int32), sizes.astype(np.int32), summary


def check(got, ref, sizes=True, summary=True):
    """Asserts the device's (labels, sizes, summary) equal to the reference's, element for element, and says what differs."""
    labels, sz, sm = (None if v is None else np.asarray(v) for v in got)
    rl, rs, rm = ref
    assert labels.shape == rl.shape and labels.dtype == np.int32
    bad = np.flatnonzero(labels != rl)
    assert not len(bad), (f"{len(bad)} labels differ; the first: particle {bad[0]} has {labels[bad[0]]}, wants {rl[bad[0]]}"
                          if len(bad) else "")
    if sizes:
        assert sz.dtype == np.int32
        bad = np.flatnonzero(sz != rs)
        assert not len(bad), f"{len(bad)} sizes differ; the first: particle {bad[0]} has {sz[bad[0]]}, wants {rs[bad[0]]}" if len(bad) else ""
    if summary:
        assert sm.dtype == np.int64 and np.array_equal(sm, rm), f"summary {sm.tolist()}, wants {rm.tolist()}"


# --------------------------------------------------------------------------------------------------------- solid bonds
def _form(ar, ai, br, bi):
    """(re_0 re'_0 + im_0 im'_0) + 2 sum_{m >= 1} (re_m re'_m + im_m im'_m), m ascending, in the arrays' type, one rounding per
    operation: the D of nl_solid_bonds."""
    s = np.zeros(len(ar), dtype=ar.dtype)
    for m in range(1, ar.shape[1]):
        s = s + (ar[:, m] * br[:, m] + ai[:, m] * bi[:, m])
    return (ar[:, 0] * br[:, 0] + ai[:, 0] * bi[:, 0]) + (s + s)


def solid_margins(qlm, I, J, thr, T):
    """(D_ij, thr sqrt(s_i s_j)) of the ordered pairs (I, J) by the rule in T from q_lm (n, l + 1) complex holding T values."""
    re, im = np.ascontiguousarray(qlm.real).astype(T), np.ascontiguousarray(qlm.imag).astype(T)
    with np.errstate(invalid="ignore"):
        s = _form(re, im, re, im)
        D = _form(re[I], im[I], re[J], im[J])
        rhs = T(thr) * np.sqrt(s[I] * s[J])
    return D, rhs


def solid_reference(ref, thr, dtype, c=None, open_pairs=()):
    """The counts' bracket of every particle from a reference of util_steinhardt.reference (its qlm, S_qlm and neighbour pairs)
    in float64: a dict of  I, J, margin, S (per ordered pair),  n_sure, n_band (n,) -- a device in `dtype` must return
    n_sure <= count <= n_sure + n_band.  open_pairs: unordered pairs (k, 2) within the band of r_max^2."""
    c = SOLID_C if c is None else c
    I, J, _ = ref["pairs"]
    q, Sq = ref["qlm"], ref["S_qlm"]
    n, l = len(q), q.shape[1] - 1
    u = lj_unit(dtype)
    D, rhs = solid_margins(q, I, J, thr, np.float64)
    w = np.where(np.arange(l + 1) == 0, 1.0, 2.0)
    a = np.abs(q.real) + np.abs(q.imag)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (w * (q.real ** 2 + q.imag ** 2)).sum(axis=1)
        A = (w * (a[J] * Sq[I, None] + a[I] * Sq[J, None])).sum(axis=1)
        Aself = 2.0 * (w * a).sum(axis=1) * Sq
        root = np.sqrt(s[I] * s[J])
        R = abs(thr) * (s[J] * Aself[I] + s[I] * Aself[J]) / (2.0 * root)
        Tij = (w * (np.abs(q.real[I] * q.real[J]) + np.abs(q.imag[I] * q.imag[J]))).sum(axis=1)
        c_qlm = us.STEIN_C["qlm"] + us.REF_C["qlm"] * 2.0 ** -53 / u  # (the reference's own q_lm error: nothing in float32)
        S = c_qlm * (A + R) + (2 * l + 4) * (Tij + abs(thr) * (s[J] * s[I] + s[I] * s[J]) / (2.0 * root)) + 3.0 * abs(thr) * root
    margin = D - rhs
    assert np.isfinite(margin).all() and np.isfinite(S).all()  # (a neighbour has neighbours: no NaN q_lm among the pairs)
    band = np.abs(margin) <= c * u * S
    extra = np.zeros(n, dtype=np.int64)
    if len(open_pairs):
        # a pair within the band of r_max^2 may or may not be a neighbour pair on the device: N_b and with it every q_lm of its two
        # particles is open, so every bond that touches one of them may go either way, and so may the pair itself
        op = np.asarray(open_pairs, dtype=np.int64).reshape(-1, 2)
        band |= np.isin(I, op) | np.isin(J, op)
        have = set(zip(I.tolist(), J.tolist()))
        for a, b in op:
            if (a, b) not in have:
                extra[a] += 1
                extra[b] += 1
    sure = (margin > 0) & ~band
    return {"I": I, "J": J, "margin": margin, "S": S, "n_sure": np.bincount(I[sure], minlength=n).astype(np.int32),
            "n_band": (np.bincount(I[band], minlength=n) + extra).astype(np.int32)}


def solid_emulate(emulated_qlm, sref, thr, T=np.float32):
    """The rule in T on the q_lm of util_steinhardt.emulate: (counts (n,), the largest |M(T) - M| / (u S) over the pairs)."""
    I, J = sref["I"], sref["J"]
    D, rhs = solid_margins(emulated_qlm, I, J, thr, T)
    dev = np.abs((D.astype(np.float64) - rhs.astype(np.float64)) - sref["margin"]) / (lj_unit(T) * sref["S"])
    counts = np.bincount(I[D > rhs], minlength=len(emulated_qlm)).astype(np.int32)
    return counts, float(dev.max(initial=0.0))


def check_solid(count, sref):
    """n_sure <= count <= n_sure + n_band for every particle."""
    count = np.asarray(count)
    assert count.dtype == np.int32 and count.shape == sref["n_sure"].shape
    bad = np.flatnonzero((count < sref["n_sure"]) | (count > sref["n_sure"] + sref["n_band"]))
    assert not len(bad), (f"{len(bad)} counts outside their bracket; the first: particle {bad[0]} has {count[bad[0]]}, wants "
                          f"{sref['n_sure'][bad[0]]} .. {sref['n_sure'][bad[0]] + sref['n_band'][bad[0]]}") if len(bad) else ""

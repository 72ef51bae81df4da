"""Reference and checker of tests/test_pair_histogram.py: the pair-distance histogram from an O(N^2) float64 sweep that uses
no list (tests.util lj_pairs), and a condition on the counts in place of a tolerance.

The checker (check_hist).  A histogram is integers: it is right or wrong.  The only freedom the contract leaves is the
rounding of r2 in the position type for a pair that sits on an edge, so for every edge k and every slot
    sure[k] <= C_got[k] <= sure[k] + m[k],     C_got[k] = sum of got[b] over b < k,
sure[k] the reference pairs with r2 < e_k^2 (1 - rho) and m[k] those with r2 within rho (relative) of e_k^2; k = nbins
included, which bounds the total.  rho = 2^-17 (fp32: the project's band for n_in and the cut-offs, 32 x the few-ulp
error of r2) or 2^-46 (fp64).  Where every m[k] = 0 this is equality, bin by bin.  At most CAP = 5 % of the reference
pairs may lie in any band: a test cannot pass by leaving its pairs undecided.
"""
import numpy as np

CAP = 0.05


def hist_rho(dtype):
    return 2.0 ** -17 if np.dtype(dtype) == np.float32 else 2.0 ** -46


def hist_edges2(r_max, nbins):
    """e_k^2, k = 0 .. nbins, with e_k = (k r_max) / nbins in double: the rule of include/nl_hip.h."""
    e = (np.arange(nbins + 1, dtype=np.float64) * float(r_max)) / float(nbins)
    return e * e


def hist_slot(a, b, ntypes):
    a, b = np.minimum(a, b), np.maximum(a, b)
    return a * (2 * ntypes - a + 1) // 2 + (b - a)


def hist_r2(pairs, n, types=None, ntypes=1, exclusions=None, rc_ab=None, without=None):
    """Sorted r2 of the pairs i < j of lj_pairs' output, one array per slot (one slot without types).  Types and
    exclusions are applied as lj_reference applies them: a pair of types with rc_ab = 0 and an excluded pair are not
    there.  without: a particle whose pairs are left out."""
    I, J, d, _ = pairs
    keep = I < J
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keys = np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]])
        keep &= ~np.isin(I * n + J, keys)
    if without is not None:
        keep &= (I != without) & (J != without)
    r2 = np.einsum("ij,ij->i", d, d)
    if types is None:
        return [np.sort(r2[keep])]
    t = np.asarray(types, dtype=np.int64)
    if rc_ab is not None:
        keep &= np.asarray(rc_ab)[t[I], t[J]] > 0
    s = hist_slot(t[I], t[J], ntypes)
    return [np.sort(r2[keep & (s == k)]) for k in range(ntypes * (ntypes + 1) // 2)]


def hist_merge(*r2_slots):
    """The reference of several frames accumulated into one histogram."""
    return [np.sort(np.concatenate(parts)) for parts in zip(*r2_slots)]


def hist_count(r2_slots, r_max, nbins):
    """(nslots, nbins) int64: the float64 histogram, E_b <= r2 < E_{b+1} with the edges unrounded."""
    e2 = hist_edges2(r_max, nbins)
    return np.stack([np.diff(np.searchsorted(r2, e2, side="left")) for r2 in r2_slots]).astype(np.int64)


def hist_bands(r2_slots, r_max, nbins, rho):
    """(sure, m), each (nslots, nbins + 1): the pairs surely below edge k, and those in its band."""
    e2 = hist_edges2(r_max, nbins)
    lo = np.stack([np.searchsorted(r2, e2 * (1.0 - rho), side="left") for r2 in r2_slots])
    hi = np.stack([np.searchsorted(r2, e2 * (1.0 + rho), side="right") for r2 in r2_slots])
    m = (hi - lo).astype(np.int64)
    m[:, 0] = 0  # (E_0 = 0 in every type: nothing lies below it, a coincident pair belongs to bin 0)
    return lo.astype(np.int64), m


def band_fraction(r2_slots, r_max, nbins, rho):
    """The share of the reference pairs below r_max (1 + rho) that lie in the band of some edge."""
    sure, m = hist_bands(r2_slots, r_max, nbins, rho)
    total = int((sure[:, -1] + m[:, -1]).sum())
    return (int(m.sum()) / total if total else 0.0), total


def check_hist(got, r2_slots, r_max, nbins, dtype, exact=None):
    """got: (nbins,) or (nslots, nbins) integers.  exact=True also demands that no pair is in a band (then the
    comparison is equality); exact=None leaves it to the input."""
    got = np.asarray(got)
    assert got.dtype.kind in "iu", got.dtype
    got = got.reshape(-1, nbins).astype(np.int64)
    assert got.shape == (len(r2_slots), nbins), (got.shape, len(r2_slots), nbins)
    assert (got >= 0).all(), "a negative counter"
    rho = hist_rho(dtype)
    frac, total = band_fraction(r2_slots, r_max, nbins, rho)
    assert frac <= CAP, f"{frac:.3%} of the {total} reference pairs lie in the band of an edge"
    sure, m = hist_bands(r2_slots, r_max, nbins, rho)
    if exact:
        assert not m.any(), f"{int(m.sum())} pairs in the band of an edge"
    C = np.concatenate([np.zeros((len(got), 1), dtype=np.int64), np.cumsum(got, axis=1)], axis=1)
    bad = np.argwhere((C < sure) | (C > sure + m))
    if len(bad):
        s, k = bad[0]
        raise AssertionError(f"slot {s}, edge {k} of {nbins}: {C[s, k]} entries below it, want {sure[s, k]} .. {sure[s, k] + m[s, k]}"
                             f" ({len(bad)} edges fail)")
    if not m.any():
        assert np.array_equal(got, hist_count(r2_slots, r_max, nbins))

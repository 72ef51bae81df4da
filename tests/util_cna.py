"""The reference of the common neighbour analysis (nl_cna): an O(N^2) float64 evaluation of the rule stated
at nl_cna in include/nl_hip.h, written from that text -- minimum image by the box matrix, candidates, ranking, both cut-off rules,
signatures by a plain graph search over Python sets, types and counts -- and the particles at which the device, which takes
every decision in the position type T, may decide otherwise (`sure` is False there).

A decision is a comparison a < b of two squared lengths.  The device's values carry a few roundings each (a separation, three
products, two adds; the adaptive Y: 14 square roots, about 14 adds, a divide and two multiplies -- well under 64 u relative), the
band is 2^-17 relative in r^2 for fp32 (u = 2^-24: 128 u) and 2^-46 for fp64 (u = 2^-53), the bands of tests/test_clusters.py.
A particle is unsure when
  * any partner's r2 lies within the band of X (a candidate may come or go, and with it N_b and the set),
  * adaptive: the ranks 11 / 12 and 13 / 14 (who is in the set) or 7 / 8 (which term is scaled by 1 / 0.75) are closer in r2
    than the band,
  * any pair of members of an analysed set has e2 within the band of Y.
"""
import numpy as np

BAND = {np.float32: 2.0 ** -17, np.float64: 2.0 ** -46}
K = 1.2071067811865475
OTHER, FCC, HCP, BCC, ICO = range(5)
MAX_NEAR = 64


def edge(r_max, dtype):
    """X: the largest T <= r_max r_max taken in double, as a float64."""
    sq = float(r_max) * float(r_max)
    if dtype == np.float64:
        return sq
    f = np.float32(sq)
    if float(f) > sq:
        f = np.nextafter(f, np.float32(0))
    return float(f)


def separations(pos, box6, mask):
    """d[i, j] = r_i - r_j at the minimum image on the axes of `mask`, (n, n, 3) float64: folded along z, then y, then x with
    the rows of the box matrix (Lx 0 0; xy Ly 0; xz yz Lz), the order of lj_image."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box6)
    d = pos[:, None, :] - pos[None, :, :]
    if mask & 4:
        k = np.rint(d[..., 2] / Lz)
        d = d - k[..., None] * np.array([xz, yz, Lz])
    if mask & 2:
        k = np.rint(d[..., 1] / Ly)
        d = d - k[..., None] * np.array([xy, Ly, 0.0])
    if mask & 1:
        k = np.rint(d[..., 0] / Lx)
        d = d - k[..., None] * np.array([Lx, 0.0, 0.0])
    return d


def _signatures(bond, members):
    """{n421, n422, n444, n555, n666} of a set: bond[k][m] says whether the members k and m are bonded."""
    n = {(4, 2, 1): 0, (4, 2, 2): 0, (4, 4, 4): 0, (5, 5, 5): 0, (6, 6, 6): 0}
    for k in members:
        common = [m for m in members if m != k and bond[k][m]]
        inner = {m: [p for p in common if p != m and bond[m][p]] for m in common}
        nb = sum(len(v) for v in inner.values()) // 2
        seen, lc = set(), 0
        for start in common:  # the connected components of (common, inner), depth first
            if start in seen:
                continue
            comp, stack = {start}, [start]
            while stack:
                for p in inner[stack.pop()]:
                    if p not in comp:
                        comp.add(p), stack.append(p)
            seen |= comp
            lc = max(lc, sum(len(inner[m]) for m in comp) // 2)
        key = (len(common), nb, lc)
        if key in n:
            n[key] += 1
    return [n[(4, 2, 1)], n[(4, 2, 2)], n[(4, 4, 4)], n[(5, 5, 5)], n[(6, 6, 6)]]


def _type12(n):
    return FCC if n[0] == 12 else HCP if (n[0] == 6 and n[1] == 6) else ICO if n[3] == 12 else OTHER


def _type14(n):
    return BCC if (n[2] == 6 and n[4] == 8) else OTHER


def _analyse(dv, Y, band):
    """(counts, sure) of the set whose members' separations from the centre are the rows of dv."""
    e = dv[:, None, :] - dv[None, :, :]
    e2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    off = ~np.eye(len(dv), dtype=bool)
    sure = not (np.abs(e2[off] / Y - 1.0) <= band).any()
    bond = (e2 < Y) & off
    return _signatures(bond.tolist(), range(len(dv))), sure


def reference(q, box6, mask, r_max, adaptive, dtype, exclusions=None):
    """{"type" (n,), "counts" (n, 8), "summary" (6,), "sure" (n,) bool} of the positions q[:, :3] (float64 holding values of
    `dtype`) in the box (Lx, Ly, Lz, xy, xz, yz) periodic on the axes of `mask`.  exclusions: (m, 2) pairs that are no
    candidates of each other."""
    pos = np.asarray(q, dtype=np.float64)[:, :3]
    n = len(pos)
    band = BAND[dtype]
    X = edge(r_max, dtype)
    d = separations(pos, box6, mask)
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    listed = ~np.eye(n, dtype=bool)
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        listed[ex[:, 0], ex[:, 1]] = listed[ex[:, 1], ex[:, 0]] = False
    types = np.zeros(n, dtype=np.int32)
    counts = np.zeros((n, 8), dtype=np.int32)
    sure = np.ones(n, dtype=bool)
    for i in range(n):
        ri = r2[i]
        cand = np.flatnonzero(listed[i] & (ri > 0) & (ri < X))
        sure[i] = not (listed[i] & (np.abs(ri / X - 1.0) <= band)).any()
        nb = len(cand)
        counts[i, 0] = nb
        if nb > MAX_NEAR:
            counts[i, 7] = 1
            continue
        if not adaptive:
            sig, ok = _analyse(d[i, cand], X, band)
            sure[i] &= ok
            counts[i, 1], counts[i, 2:7] = nb, sig
            types[i] = _type12(sig) if nb == 12 else _type14(sig) if nb == 14 else OTHER
            continue
        if nb < 12:
            continue
        order = cand[np.lexsort((cand, ri[cand]))]  # by (r2, j)
        rr = ri[order]

        def apart(a, b):
            return b >= nb or abs(rr[a] / rr[b] - 1.0) > band

        sure[i] &= apart(11, 12)
        S = 0.0
        for t in range(12):
            S += np.sqrt(rr[t])
        c = (S / 12.0) * K
        sig, ok = _analyse(d[i, order[:12]], c * c, band)
        sure[i] &= ok
        counts[i, 1], counts[i, 2:7] = 12, sig
        types[i] = _type12(sig)
        if types[i] != OTHER or nb < 14:
            continue
        sure[i] &= apart(13, 14) and apart(7, 8)
        S = 0.0
        for t in range(14):
            S += np.sqrt(rr[t] / 0.75) if t < 8 else np.sqrt(rr[t])
        c = (S / 14.0) * K
        sig, ok = _analyse(d[i, order[:14]], c * c, band)
        sure[i] &= ok
        counts[i, 1], counts[i, 2:7] = 14, sig
        types[i] = _type14(sig)
    summary = np.zeros(6, dtype=np.int64)
    summary[:5] = np.bincount(types, minlength=5)
    summary[5] = int(counts[:, 7].sum())
    return {"type": types, "counts": counts, "summary": summary, "sure": sure}


def check(got_type, got_counts, got_summary, ref, what=""):
    """The device's outputs against the reference: type and all eight counts words at every sure particle, the summary against
    the histogram of the device's own types at all particles, and word 5 against the device's own flags."""
    s = ref["sure"]
    bad = np.flatnonzero(s & (got_type != ref["type"]))
    assert not len(bad), (what, "types differ at", bad[:8].tolist(), got_type[bad[:8]].tolist(), ref["type"][bad[:8]].tolist())
    if got_counts is not None:
        bad = np.flatnonzero(s & (got_counts != ref["counts"]).any(axis=1))
        assert not len(bad), (what, "counts differ at", bad[:4].tolist(), got_counts[bad[:4]].tolist(), ref["counts"][bad[:4]].tolist())
    if got_summary is not None:
        assert got_type.min() >= 0 and got_type.max() <= 4
        assert np.array_equal(got_summary[:5], np.bincount(got_type, minlength=5)), (what, got_summary.tolist())
        if got_counts is not None:
            assert got_summary[5] == (got_counts[:, 7] & 1).sum(), (what, got_summary.tolist())
        if s.all():
            assert np.array_equal(got_summary, ref["summary"]), (what, got_summary.tolist(), ref["summary"].tolist())

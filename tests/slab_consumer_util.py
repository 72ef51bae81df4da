"""What tests/test_slab_consumers.py checks the consumers of a local-index slab list against (nl_set_local_ids, DESIGN.md
section 8n): one rank's share of the forces, the virial totals and the pair histogram, from the O(N^2) float64 pairs of the
global box (tests.util lj_pairs) and the slabs of tests.test_slab_paths.slab_parts.  No list is used, the library's or the
oracle's.  The rule per ordered pair (i owned, j), j a ghost iff this rank does not own it:
  forces     the owned rows of the global sum: every pair of an owned particle acts on it, a ghost receives nothing here;
  virial     weight 1/2 for every ordered pair, which is 1 per owned-owned pair and 1/2 per owned-ghost pair;
  histogram  an owned-owned pair once; an owned-ghost pair iff dz < 0, or dz == 0 and z_i < z_j as given (d = r_i - r_j).
Each function can be told to break its rule in one way (ghost_reaction, ghost_weight, crossing): the tests show that the
checkers reject every one of them."""
import numpy as np

from tests.util import lj_reference
from tests.virial_util import virial_rows


def within(pairs, n, rmax, exclusions=None):
    """The ordered pairs of lj_pairs' output with 0 < r < rmax, without the excluded ones ((E, 2), either order)."""
    I, J, d, raw = pairs
    r2 = np.einsum("ij,ij->i", d, d)
    keep = (r2 > 0) & (r2 < rmax * rmax)
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keys = np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]])
        keep &= ~np.isin(I * n + J, keys)
    return I[keep], J[keep], d[keep], raw[keep]


def rank_split(pairs, n, part):
    """(owned-owned, owned-ghost, uncovered): the ordered pairs (i, j) with i owned by the slab `part`, by what j is to it;
    uncovered counts those whose partner the slab does not hold at all."""
    I, J, d, raw = pairs
    own = np.zeros(n, dtype=bool)
    own[part["own"]] = True
    held = np.zeros(n, dtype=bool)
    held[part["order"]] = True
    mine = own[I]
    oo, og = mine & own[J], mine & ~own[J]
    pick = lambda m: (I[m], J[m], d[m], raw[m])  # noqa: E731
    return pick(oo), pick(og), int((mine & ~held[J]).sum())


def rank_forces(q, box6, mask, rcf, pairs, part, exclusions=None, ghost_reaction=False):
    """(want[n_rows, 4], S[n_rows, 4]) of the slab's owned rows, summed from the rank's own pairs.  ghost_reaction (wrong):
    the reaction of every owned-ghost pair comes back from the ghost's owner as well, as reverse communication would add it."""
    n = len(q)
    inside = within(pairs, n, rcf, exclusions)
    own = np.zeros(n, dtype=bool)
    own[part["own"]] = True
    mine = tuple(v[own[inside[0]]] for v in inside)  # (in the order of the global sum: the rows come out bit for bit)
    if ghost_reaction:
        mine = tuple(np.concatenate([a, b]) for a, b in zip(mine, rank_split(inside, n, part)[1]))
    want, S = lj_reference(q, box6, mask, 1.0, 1.0, rcf, pairs=mine)
    return want[part["own"]], S[part["own"]]


def rank_virial(n, rcf, pairs, part, exclusions=None, ghost_weight=0.5):
    """(want[8], S[7]) of the slab: 1/2 per ordered owned-owned pair (1 per pair), ghost_weight per owned-ghost pair -- 1/2,
    since the ghost's owner holds the other half; 1 is the wrong rule that counts a crossing pair in full on both ranks."""
    oo, og, _ = rank_split(within(pairs, n, rcf, exclusions), n, part)
    want, S = np.zeros(8), np.zeros(7)
    for (I, _, d, _), w in ((oo, 0.5), (og, ghost_weight)):
        one = np.ones(len(I))
        row, S_row = virial_rows(n, I, d, one, one)
        want[:7] += w * row.sum(axis=0)
        want[7] += w * len(I)
        S += w * S_row.sum(axis=0)
    return want, S


def rank_hist_r2(q, n, r_top, pairs, part, exclusions=None, crossing="first"):
    """[sorted r2] (one slot, the form of tests.hist_util) of the pairs the slab counts, up to r_top.  crossing: which rank
    counts a pair that crosses a cut -- "first" (the rule), "both" or "none" (wrong)."""
    I, J, d, raw = pairs
    r2 = np.einsum("ij,ij->i", d, d)
    keep = r2 < r_top * r_top  # (a coincident pair belongs to bin 0: not `within`)
    if exclusions is not None and len(exclusions):
        ex = np.asarray(exclusions, dtype=np.int64)
        keys = np.concatenate([ex[:, 0] * n + ex[:, 1], ex[:, 1] * n + ex[:, 0]])
        keep &= ~np.isin(I * n + J, keys)
    oo, og, _ = rank_split((I[keep], J[keep], d[keep], raw[keep]), n, part)
    z = np.asarray(q)[:, 2]
    gi, gj, gd, _ = og
    first = (gd[:, 2] < 0) | ((gd[:, 2] == 0) & (z[gi] < z[gj]))
    take = {"first": first, "both": np.ones(len(gi), dtype=bool), "none": np.zeros(len(gi), dtype=bool)}[crossing]
    once = oo[0] < oo[1]
    return [np.sort(np.concatenate([np.einsum("ij,ij->i", oo[2][once], oo[2][once]), np.einsum("ij,ij->i", gd[take], gd[take])]))]


def local_pairs(pairs_global, part, n):
    """(E, 2) global id pairs in the rows of the slab's buffer (owned first, then the two ghost layers); a pair with a
    particle the slab does not hold is left out."""
    loc = np.full(n, -1, dtype=np.int64)
    loc[part["order"]] = np.arange(len(part["order"]))
    p = loc[np.asarray(pairs_global, dtype=np.int64)]
    return p[(p >= 0).all(axis=1)].astype(np.int32)

#!/usr/bin/env python3
"""tools/reach_cull_model.py [n] [cells]: what the reach cull (cls_cull, NL_CULL) removes from the staged stream of an
id-class build, counted on the CPU for a uniform box of cfg 2's density (rho = 1, rc = 3.3; default n = 2^20, 400
sampled interior cells, random ids, two classes).

reach = a slot is kept if its squared distance to the box is at most rc^2, for two boxes: the cell's geometric box
(what the proposal was sized with) and the bounding box of the cell's own particles (what the kernel uses: tighter, and
it covers particles filed into an edge cell from outside the box).  Tiles: a class-0 group walks the whole stream, a
class-1 group from the tile its class starts in."""
import sys

import numpy as np

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
samples = int(sys.argv[2]) if len(sys.argv) > 2 else 400
rng = np.random.default_rng(7)
L = n ** (1 / 3)
rc = 3.3
M = int(L / rc)
ms = L / M
q = rng.random((n, 3)) * L
ids = rng.permutation(n)
c = np.minimum((q / ms).astype(int), M - 1)
key = (c[:, 2] * M + c[:, 1]) * M + c[:, 0]
order = np.argsort(key, kind="stable")
qs, ks, idsr = q[order], key[order], ids[order]
start = np.searchsorted(ks, np.arange(M ** 3 + 1))


def cell(x, y, z):
    k = (z * M + y) * M + x
    return slice(start[k], start[k + 1])


rows = {"cell box": [], "particle box": []}
for _ in range(samples):
    cx, cy, cz = rng.integers(1, M - 1, 3)
    own = qs[cell(cx, cy, cz)]
    if len(own) == 0:
        continue
    boxes = {"cell box": (np.array([cx, cy, cz]) * ms, (np.array([cx, cy, cz]) + 1) * ms),
             "particle box": (own.min(axis=0), own.max(axis=0))}
    for name, (lo, hi) in boxes.items():
        tot, kept = [0, 0], [0, 0]
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    s = cell(cx + dx, cy + dy, cz + dz)
                    p, cl = qs[s], (idsr[s] >= n // 2).astype(int)
                    d = np.maximum(np.maximum(lo - p, p - hi), 0)
                    k = (d * d).sum(1) <= rc * rc
                    for a in (0, 1):
                        tot[a] += (cl == a).sum()
                        kept[a] += ((cl == a) & k).sum()
        T, K = sum(tot), sum(kept)
        nt, ntk = -(-T // 64), -(-K // 64)
        rows[name].append((T, K, nt, nt - tot[0] // 64, ntk, ntk - kept[0] // 64))
print(f"mesh {M}^3, cell edge {ms:.4f} = {ms / rc:.4f} rc, {n / M ** 3:.1f} particles per cell")
for name, r in rows.items():
    r = np.array(r, float)
    print(f"-- reach from the {name}")
    print(f"stream per cell {r[:, 0].mean():.0f} -> {r[:, 1].mean():.0f} ({r[:, 1].mean() / r[:, 0].mean():.3f})")
    print(f"tiles walked, class 0 {r[:, 2].mean():.1f} -> {r[:, 4].mean():.1f}, class 1 {r[:, 3].mean():.1f} -> {r[:, 5].mean():.1f}")
    both, both_k = (r[:, 2] + r[:, 3]).mean(), (r[:, 4] + r[:, 5]).mean()
    print(f"tile steps per class-0 + class-1 pair {both:.1f} -> {both_k:.1f} ({both_k / both:.3f})")
    print(f"cells with more than 16 tiles {(r[:, 2] > 16).mean():.0%} -> {(r[:, 4] > 16).mean():.0%} (most kept tiles: {r[:, 4].max():.0f})")

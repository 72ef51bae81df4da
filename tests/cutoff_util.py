"""Adversarial input for the cut-off decision (tests/test_cutoff_paths.py): pairs constructed at distance rc (1 + k ulp)
in the placements where a search kernel's shortcut has no slack, and the decision rule of include/nl_hip.h restated in
numpy for those pairs.

The contract: a pair is in the list iff !(r2 > rc2), r2 = (dx*dx + dy*dy) + dz*dz rounded operation by operation in the
position type T, at the image the header prescribes (nl_set_periodic_axes): on an axis of the mask a particle whose cell
index wrapped is stored at q -+ (T)L, and a partner staged through a face is shifted by -+ (T)L, rounded to T, before the
difference is taken; on an open axis the coordinates are used as given.  rule_r2 evaluates exactly that for chosen
(row, partner) pairs; the lists themselves always come from the oracle.
"""
import numpy as np

RC = 3.3
BOX = (16.6, 19.95, 16.6)  # 5 x 6 x 5 cells, ms_z / rc = 1.00606
PAIRS = 400                # constructed pairs per class
BLOB_N, BLOB_EDGE = 700, 2.5
FACE = {"face_x": 0, "face_y": 1, "face_z": 2}
OUTSIDE = {"outside_x": 0, "outside_y": 1, "outside_z": 2}
CLASSES = ("rand", "corner", "zplane", "cluster", "cut") + tuple(FACE) + tuple(OUTSIDE)


def mesh(box, rc=RC):
    return tuple(int(b / rc) for b in box)


def grid(box, rc, dtype):
    """(m, ms, ims, L): the mesh, and cell edge, its inverse and the box rounded to T as nl_create rounds them."""
    T = np.dtype(dtype).type
    m = np.array(mesh(box, rc), dtype=np.int64)
    ms = (np.asarray(box, dtype=np.float64) / m).astype(T)
    ims = (1.0 / ms.astype(np.float64)).astype(T)
    return m, ms, ims, np.asarray(box, dtype=np.float64).astype(T)


def stored(q, box, rc, mask):
    """(cell index [n, 3], stored coordinate [n, 3] in T) of every particle: on an axis of the mask the floor of q * ims,
    one wrap, and the image q -+ L next to that cell; on an open axis the reference's truncation, one wrap, q as given."""
    T = q.dtype.type
    m, _, ims, L = grid(box, rc, T)
    p = np.ascontiguousarray(q[:, :3])
    t = p * ims
    assert t.dtype == q.dtype
    per = np.array([bool(mask >> d & 1) for d in range(3)])
    c = np.where(per, np.floor(t), np.trunc(t)).astype(np.int64)
    lo, hi = c < 0, c >= m
    e = np.where(per & lo, p + L, np.where(per & hi, p - L, p)).astype(T)
    c = c + np.where(lo, m, 0) - np.where(hi, m, 0)
    assert np.all((c >= 0) & (c < m)), "a coordinate more than one box length outside [0, L)"
    return c, e


def rule_r2(q, rows, cols, box, rc, mask):
    """(r2 in T, visited) for the entries (row i, partner j): the r2 the header prescribes for row i, and whether j's cell
    is one of the 27 around i's (the stencil wraps on every axis; it shifts only on the axes of the mask)."""
    T = q.dtype.type
    m, _, _, L = grid(box, rc, T)
    c, e = stored(q, box, rc, mask)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    visited = np.ones(len(rows), dtype=bool)
    d = []
    for a in range(3):
        off = c[cols, a] - c[rows, a]
        visited &= (np.abs(off) <= 1) | (np.abs(off) == m[a] - 1)
        xj = e[cols, a]
        if mask >> a & 1:  # i in the first cell and j in the last: j is staged at -L; the other way round at +L
            xj = np.where(off == m[a] - 1, xj - L[a], np.where(off == 1 - m[a], xj + L[a], xj)).astype(T)
        d.append(xj - e[rows, a])
    r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert r2.dtype == q.dtype
    return r2, visited


def brute_force(q, box, rc, mask, chunk=256):
    """The full list by the header's rule over all n^2 ordered pairs, row i in its own frame: (counts[n], key_pointer[n + 1],
    partners ascending per row).  Admits whatever coordinates the library admits (up to a box length outside on every side),
    which the padded reference of tests/test_periodic_axes.py does not on an open axis; tests/test_cutoff_paths.py checks
    it against the oracle's lists wherever those exist.  The half list is its entries with j > i."""
    T = q.dtype.type
    m, _, _, L = grid(box, rc, T)
    c, e = stored(q, box, rc, mask)
    n, rc2 = len(q), rc * rc
    rows, cols = [], []
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        ok = np.ones((i1 - i0, n), dtype=bool)
        sq = []
        for a in range(3):
            off = c[None, :, a] - c[i0:i1, None, a]
            ok &= (np.abs(off) <= 1) | (np.abs(off) == m[a] - 1)
            xj = e[None, :, a]
            if mask >> a & 1:
                xj = np.where(off == m[a] - 1, xj - L[a], np.where(off == 1 - m[a], xj + L[a], xj))
            d = xj - e[i0:i1, None, a]
            assert d.dtype == q.dtype
            sq.append(d * d)
        r2 = (sq[0] + sq[1]) + sq[2]
        ok &= ~(r2.astype(np.float64) > rc2)
        ok[np.arange(i1 - i0), np.arange(i0, i1)] = False
        r, j = np.nonzero(ok)
        rows.append(r + i0)
        cols.append(j)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    cnt = np.bincount(rows, minlength=n)
    return cnt, np.concatenate([[0], np.cumsum(cnt)]), cols.astype(np.int64)


def accepted(q, rows, cols, box, rc, mask):
    r2, visited = rule_r2(q, rows, cols, box, rc, mask)
    return visited & ~(r2.astype(np.float64) > rc * rc)


def near_cutoff(r2, rc, ulps=16):
    """|r2 - rc2| <= ulps ulp_T(rc2), rc2 = rc * rc in double as the handle holds it."""
    rc2 = rc * rc
    return np.abs(r2.astype(np.float64) - rc2) <= ulps * float(np.spacing(r2.dtype.type(rc2)))


def quarter_index(q, box, rc):
    """4 * cell + quarter along z of every particle: the quarter is the fraction of the product that the reference
    truncates (the rule of test_hash_and_sort_stage)."""
    T = q.dtype.type
    _, _, ims, _ = grid(box, rc, T)
    t = q[:, 2] * ims[2]
    frac = t - np.trunc(t)
    return 4 * np.trunc(t).astype(np.int64) + np.clip(np.floor(frac * T(4.0)), 0, 3).astype(np.int64)


def blob_origin(box, rc=RC):
    """The blob of the `cluster` class fills a cube of BLOB_EDGE inside the cell (2, 3, 2)."""
    m = mesh(box, rc)
    return np.array([2 * box[0] / m[0], 3 * box[1] / m[1], 2 * box[2] / m[2]]) + 0.4


def _scales(n, dtype, rng):
    if np.dtype(dtype) == np.float32:
        return 1.0 + rng.integers(-6, 7, size=n) * 2.0 ** -23
    k52 = rng.integers(-8, 9, size=n) * 2.0 ** -52
    k24 = rng.integers(-96, 97, size=n) * 2.0 ** -24
    return 1.0 + np.where(rng.permutation(n) % 2 == 0, k52, k24)  # (half of each, independent of the placement)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _through(n, axis, sign, rng):
    """Unit vectors whose component along `axis` is sign * U(0.6, 0.95), the rest a random direction in the plane."""
    d = np.zeros((n, 3))
    d[:, axis] = sign * rng.uniform(0.6, 0.95, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    lat = np.sqrt(1.0 - d[:, axis] ** 2)
    d[:, (axis + 1) % 3], d[:, (axis + 2) % 3] = lat * np.cos(phi), lat * np.sin(phi)
    return d


def cloud(box, rc, dtype, mask, classes, rng, per_cell=30.0, pairs=PAIRS, cuts=(2, 4), with_pairs=False, nonneg_open=False):
    """Positions (n, 4) in `dtype`: constructed pairs (c, c + d rc s) of every class of `classes`, `pairs` of each, and
    uniform background particles that fill the box up to `per_cell` particles per cell in all (the density that selects
    the search path); shuffled, so that ids do not correlate with the construction.

    s = 1 + k 2^-23, k in [-6, 6] (fp32); fp64: half the pairs k 2^-52, k in [-8, 8], the other half k 2^-24, k in
    [-96, 96], on both sides of the fp64 screen's band edges.  The centre c is rounded to T first and the partner is
    the double expression rounded to T once.  Classes:
      rand       uniform centres, random direction
      corner     centres at fractions 0.002 / 0.998 of their cell on every axis, a roughly diagonal direction into the
                 (+-1, +-1, +-1) stencil cell: the largest R_i + R_j of the fp64 screen
      zplane     direction along +-z (lateral components 1e-4 .. 1e-3 of the length), the centre's z within +-4 ulp of a
                 quarter-plane of its cell: the reach q - 4 .. q + 4 of the fine rows
      face_x/y/z centres within rc / 2 of the low or high face, direction through it; every second partner is left outside
                 [0, L), the others are wrapped in by one rounded operation in T
      outside_*  the centre moved by a whole -L or +L on that axis and rounded to T, the partner built from the rounded
                 centre: open axes only
      cluster    a blob of BLOB_N background particles in a cube of BLOB_EDGE inside one cell, pairs with centres in it
      cut        as face_z, through the planes between the z layers `cuts` and the layers below them (slab boundaries)
    nonneg_open: no coordinate of an open axis is negative, which the padded reference of tests/test_periodic_axes.py
    requires of a mixed mask: outside_* moves by +L only, and a partner that a low open face would leave at a negative
    coordinate is wrapped in instead.
    with_pairs: also returns {"a": centre ids, "b": partner ids, "cls": class name per pair}."""
    T = np.dtype(dtype).type
    L = np.asarray(box, dtype=np.float64)
    m = np.array(mesh(box, rc))
    ms = L / m
    LT = L.astype(T).astype(np.float64)
    mixed = bool(nonneg_open)
    inner_lo, inner_hi = 1.01 * rc, L - 1.01 * rc
    cen, par, names = [], [], []

    def emit(name, c, d, fix=None):
        c = c.astype(T).astype(np.float64)
        p = (c + d * rc * _scales(len(c), T, rng)[:, None]).astype(T)
        if fix is not None:
            p = fix(p)
        cen.append(c.astype(T))
        par.append(p.astype(T))
        names.extend([name] * len(c))

    for name in classes:
        n = pairs
        if name == "rand":
            emit(name, rng.uniform(inner_lo, inner_hi, (n, 3)), _unit(rng.normal(size=(n, 3))))
        elif name == "corner":
            hi = rng.integers(0, 2, (n, 3))
            cell = np.stack([rng.integers(1, m[a] - 1, n) for a in range(3)], axis=1)
            c = (cell + np.where(hi, 0.998, 0.002)) * ms
            emit(name, c, _unit(rng.uniform(0.35, 0.75, (n, 3)) * np.where(hi, 1.0, -1.0)))
        elif name == "zplane":
            c = rng.uniform(inner_lo, inner_hi, (n, 3))
            z = ((rng.integers(1, m[2] - 1, n) + rng.integers(0, 4, n) / 4.0) * ms[2]).astype(T)
            z = z + rng.integers(-4, 5, n).astype(T) * np.spacing(z)
            assert z.dtype == np.dtype(T)
            c[:, 2] = z
            d = np.zeros((n, 3))
            d[:, :2] = rng.uniform(1e-4, 1e-3, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
            d[:, 2] = np.sqrt(1.0 - d[:, 0] ** 2 - d[:, 1] ** 2) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
            emit(name, c, d)
        elif name in FACE or name == "cut":
            a = 2 if name == "cut" else FACE[name]
            high = np.arange(n) % 2 == 1
            wrap = np.arange(n) // 2 % 2 == 1
            c = rng.uniform(inner_lo, inner_hi, (n, 3))
            near = rng.uniform(0.05, 0.45, n) * rc
            if name == "cut":
                plane = np.asarray(cuts)[rng.integers(0, len(cuts), n)] * ms[2]
                c[:, a] = np.where(high, plane - near, plane + near)
                emit(name, c, np.where(high[:, None], _through(n, a, 1.0, rng), _through(n, a, -1.0, rng)))
                continue
            c[:, a] = np.where(high, L[a] - near, near)
            if mixed and not mask >> a & 1:
                wrap = wrap | ~high

            def fix(p, a=a, high=high, wrap=wrap):
                s = np.where(high, -T(LT[a]), T(LT[a])).astype(T)
                p[:, a] = np.where(wrap, p[:, a] + s, p[:, a])  # (one rounded operation in T)
                assert p.dtype == np.dtype(T)
                return p

            emit(name, c, np.where(high[:, None], _through(n, a, 1.0, rng), _through(n, a, -1.0, rng)), fix)
        elif name in OUTSIDE:
            a = OUTSIDE[name]
            assert not mask >> a & 1, "outside_*: open axes only"
            c = rng.uniform(inner_lo, inner_hi, (n, 3)).astype(T)
            up = np.ones(n, dtype=bool) if mixed else np.arange(n) % 2 == 1
            c[:, a] = c[:, a] + np.where(up, T(LT[a]), -T(LT[a])).astype(T)
            assert c.dtype == np.dtype(T)
            emit(name, c.astype(np.float64), _unit(rng.normal(size=(n, 3))))
        elif name == "cluster":
            emit(name, blob_origin(box, rc) + rng.uniform(0.0, BLOB_EDGE, (n, 3)), _unit(rng.normal(size=(n, 3))))
        else:
            raise ValueError(name)

    built = 2 * pairs * len(classes) + (BLOB_N if "cluster" in classes else 0)
    nbg = int(round(per_cell * int(np.prod(m)))) - built
    assert nbg >= 0, (per_cell, built)
    bg = np.minimum((rng.uniform(0.0, 1.0, (nbg, 3)) * L).astype(T), np.nextafter(L.astype(T), T(0)))
    parts = cen + par + [bg]
    if "cluster" in classes:
        parts.append((blob_origin(box, rc) + rng.uniform(0.0, BLOB_EDGE, (BLOB_N, 3))).astype(T))
    pos = np.concatenate(parts)
    npair = len(names)
    perm = rng.permutation(len(pos))  # new id of every constructed row
    q = np.zeros((len(pos), 4), dtype=T)
    q[perm, :3] = pos
    if not with_pairs:
        return q
    return q, {"a": perm[:npair], "b": perm[npair:2 * npair], "cls": np.array(names)}

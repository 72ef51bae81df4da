"""Common neighbour analysis, host side of nl_cna (include/nl_hip.h).

NeighListGPU.cna() gives every particle one of the types below; the helpers here name them, turn them into fractions, give the
conventional cut-offs of the fixed mode and generate the ideal structures the analysis recognises:

NAMES, OTHER .. ICO          the types, OVITO's numbering
fractions(types)             {name: fraction of the particles}
default_r_max(kind, a)       the conventional fixed cut-off of a lattice with lattice constant a
lattice(kind, cells, a)      ideal fcc, bcc (cubic cells of edge a) or hcp (orthorhombic cells, a the neighbour distance)
stacked(sequence, nx, ny, d) close-packed layers stacked along z in any order: "ABC" fcc, "AB" hcp, "ABCABCBCABC" an fcc
                             crystal with one intrinsic stacking fault
icosahedron(r)               the 13-atom icosahedron, its centre first

For the adaptive mode no cut-off has to be chosen: any ``r_max`` that holds at least 14 neighbours of every particle and at most
64 serves (about 1.2 to 1.6 nearest-neighbour distances in a dense phase).
"""
import numpy as np

OTHER, FCC, HCP, BCC, ICO = 0, 1, 2, 3, 4
NAMES = ("other", "fcc", "hcp", "bcc", "ico")
MAX_NEAR = 64


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def fractions(types):
    """``{name: fraction}`` of the particles of every type of NAMES; ``types`` a device tensor or anything numpy takes.  A
    type below 0 (a failed list) counts for none."""
    t = types.detach().cpu().numpy() if _is_tensor(types) else np.asarray(types)
    t = t.astype(np.int64).reshape(-1)
    n = max(len(t), 1)
    cnt = np.bincount(t[(t >= 0) & (t < len(NAMES))], minlength=len(NAMES))
    return {name: float(c) / n for name, c in zip(NAMES, cnt)}


def default_r_max(kind, a):
    """The conventional cut-off of the fixed mode.  fcc (``a``: the cubic lattice constant) and hcp (``a``: the
    neighbour distance, the hexagonal lattice constant): midway between the first and the second shell.  bcc (``a``: the
    cubic lattice constant): ``(1 + sqrt 2) / 2 a``, midway between the second and the third shell."""
    kind = kind.lower()
    if kind == "fcc":
        return 0.5 * (np.sqrt(0.5) + 1.0) * a
    if kind in ("hcp", "bcc"):
        return 0.5 * (1.0 + np.sqrt(2.0)) * a
    raise ValueError("kind must be 'fcc', 'hcp' or 'bcc'")


def lattice(kind, cells, a=1.0):
    """``(positions (n, 3), box lengths (3,))`` of a perfect periodic lattice of ``cells`` (an int or three) cells: cubic cells
    of edge ``a`` with 4 (fcc) or 2 (bcc) atoms, or the orthorhombic hcp cell ``(a, a sqrt 3, a sqrt(8 / 3))`` of 4 atoms with
    the neighbour distance ``a``."""
    kind = kind.lower()
    cells = np.broadcast_to(np.asarray(cells, dtype=np.int64), (3,))
    if kind == "hcp":
        cell = a * np.array([1.0, np.sqrt(3.0), np.sqrt(8.0 / 3.0)])
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 5.0 / 6.0, 0.5], [0, 1.0 / 3.0, 0.5]])
    elif kind == "fcc":
        cell = a * np.ones(3)
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], dtype=np.float64)
    elif kind == "bcc":
        cell = a * np.ones(3)
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0.5]], dtype=np.float64)
    else:
        raise ValueError("kind must be 'fcc', 'hcp' or 'bcc'")
    g = np.stack(np.meshgrid(*(np.arange(c) for c in cells), indexing="ij"), axis=-1).reshape(-1, 1, 3)
    return ((g + basis[None, :, :]) * cell).reshape(-1, 3), cells * cell


def stacked(sequence, nx, ny, d=1.0):
    """``(positions (n, 3), box lengths (3,), layer (n,))``: close-packed (triangular) layers of neighbour distance ``d``,
    ``nx`` by ``ny`` orthorhombic cells ``(d, d sqrt 3)`` of two atoms each, stacked along z at ``d sqrt(2 / 3)`` in the
    positions ``sequence`` names, a string of A, B, C read cyclically (the box is periodic along z as well): neighbouring letters
    must differ, the last and the first included.  ``layer``: the index of every atom's layer.  A layer between two different
    letters is fcc, between two equal ones hcp."""
    seq = sequence.upper()
    if len(seq) < 2 or any(c not in "ABC" for c in seq) or any(seq[k] == seq[(k + 1) % len(seq)] for k in range(len(seq))):
        raise ValueError("sequence: letters A, B, C, neighbours different, cyclically")
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    base = np.stack([gx.ravel(), gy.ravel() * np.sqrt(3.0)], axis=1).astype(np.float64)
    plane = np.concatenate([base, base + np.array([0.5, 0.5 * np.sqrt(3.0)])]) * d
    h = d * np.sqrt(2.0 / 3.0)
    pos, layer = [], []
    for k, c in enumerate(seq):
        p = np.zeros((len(plane), 3))
        p[:, :2] = plane
        p[:, 1] += "ABC".index(c) * d / np.sqrt(3.0)
        p[:, 2] = k * h
        pos.append(p), layer.append(np.full(len(plane), k))
    box = np.array([nx * d, ny * d * np.sqrt(3.0), len(seq) * h])
    pos = np.concatenate(pos)
    pos[:, 1] %= box[1]
    return pos, box, np.concatenate(layer)


def icosahedron(r=1.0):
    """``(13, 3)``: the centre at the origin, then the 12 vertices of an icosahedron at the distance ``r`` (neighbouring
    vertices are 1.0515 r apart)."""
    phi = 0.5 * (1.0 + np.sqrt(5.0))
    v = [(0.0, s1, s2 * phi) for s1 in (-1, 1) for s2 in (-1, 1)]
    v = v + [(y, z, x) for x, y, z in v] + [(z, x, y) for x, y, z in v]
    v = np.array(v) * (r / np.sqrt(1.0 + phi * phi))
    return np.concatenate([np.zeros((1, 3)), v])

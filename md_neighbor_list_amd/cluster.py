"""Clusters from the list, host side of nl_clusters and nl_solid_bonds (include/nl_hip.h).

NeighListGPU.clusters() labels every member with the smallest particle index of its cluster; the helpers here turn those labels
into what an analysis reports:

relabel_by_size(labels)     freud's numbering: 0 .. k - 1 by descending size, ties by label, non-members -1
size_distribution(labels)   (sizes, counts): the distinct cluster sizes, ascending, and how many clusters have each
solid_liquid(nl, q, ...)    the ten Wolde-Frenkel pipeline: steinhardt -> solid_bonds -> clusters of the solid particles

Labels may be a device tensor (the work stays on the device and a tensor comes back) or anything numpy takes.
"""
import numpy as np


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def relabel_by_size(labels):
    """Cluster numbers 0 .. k - 1 in the order of descending size, clusters of equal size in the order of their labels, -1 for a
    non-member (label < 0): the numbering of freud.cluster.Cluster.  int32, a tensor for a tensor, an array otherwise."""
    if _is_tensor(labels):
        import torch

        lab = labels.to(torch.int64)
        m = lab >= 0
        uniq, inv, cnt = torch.unique(lab[m], return_inverse=True, return_counts=True)  # (uniq ascending)
        order = torch.sort(cnt, descending=True, stable=True).indices
        rank = torch.empty_like(order)
        rank[order] = torch.arange(len(order), device=order.device)
        out = torch.full_like(lab, -1)
        out[m] = rank[inv]
        return out.to(torch.int32)
    lab = np.asarray(labels, dtype=np.int64)
    m = lab >= 0
    uniq, inv, cnt = np.unique(lab[m], return_inverse=True, return_counts=True)
    order = np.argsort(-cnt, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    out = np.full(lab.shape, -1, dtype=np.int32)
    out[m] = rank[inv.reshape(-1)]
    return out


def size_distribution(labels):
    """``(sizes, counts)`` as int64 arrays on the host: the distinct cluster sizes in ascending order and the number of
    clusters of each size.  ``(sizes * counts).sum()`` is the number of members."""
    lab = labels.detach().cpu().numpy() if _is_tensor(labels) else np.asarray(labels)
    lab = lab.astype(np.int64)
    per_cluster = np.unique(lab[lab >= 0], return_counts=True)[1]
    sizes, counts = np.unique(per_cluster, return_counts=True)
    return sizes.astype(np.int64), counts.astype(np.int64)


def solid_liquid(nl, q, l=6, r_max=None, threshold=0.7, n_min=7, wait=True):
    """Solid-like particles and their clusters after ten Wolde, Ruiz-Montero and Frenkel, on the full list ``nl`` holds of the
    positions ``q``: sets the Steinhardt degree ``l`` and range ``r_max`` where the handle's setting differs (its w_l table
    is dropped then), calls steinhardt(), counts every particle's neighbours j with
    ``q_l(i) . q_l(j) > threshold |q_l(i)| |q_l(j)|`` (solid_bonds), and clusters the particles with at least ``n_min`` such
    bonds within ``r_max`` of each other (clusters).  ``wait=False`` uses the enqueue variants throughout.  Returns a dict of
    device tensors: ``order`` (n, 4) of steinhardt(), ``solid_bonds`` (n,), ``labels`` (n,), ``sizes`` (n,) and ``summary``
    (4,) = {solid particles, clusters, size of the largest cluster, its label}."""
    if r_max is None:
        raise ValueError("solid_liquid() needs the neighbour range r_max")
    info = nl.steinhardt_info()
    if info is None or info["l"] != int(l) or info["r_max"] != float(r_max):
        nl.set_steinhardt(l, r_max, w=False)
    order = nl.steinhardt(q, average=False, wait=wait)
    bonds = nl.solid_bonds(q, threshold, wait=wait)
    labels, sizes, summary = nl.clusters(q, r_max, member=bonds, min_member=int(n_min), wait=wait)
    return {"order": order, "solid_bonds": bonds, "labels": labels, "sizes": sizes, "summary": summary}

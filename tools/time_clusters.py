#!/usr/bin/env python3
"""What do nl_clusters and nl_solid_bonds cost against the histogram of the same list?  fp32, N = 2^20
uniform particles at rho = 1, one handle and one full list per workload:
  cfg2    rc = 3.3 (about 150 entries a row, half of them used): the walk dominates, edges are a few per cent of the entries
  tight   rc = 1.6 (about 17 entries a row): the entries that are edges are a large share
nl_clusters at r_max = 0.75, below the continuum percolation threshold (0.868 at rho = 1: many small clusters), and at 1.1, above
it (one giant cluster: the longest paths and the most failed CAS), each with sizes and summary; nl_solid_bonds at l = 6 on the
q_lm of one nl_steinhardt call at r_max = 1.5.  The yardstick runs on the same list in the same process: nl_pair_histogram to the
same r_max (the same walk; its per-entry work is an LDS atomic).  The tool first checks the answers' invariants (sizes add up to
the members, the giant cluster is there or not).  Interleaved batches: every batch times each of the calls REPS times back to back
between two events; the figure is the median over the batches of the batch's mean, with the spread of the batches beside it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, cluster, inputs  # noqa: E402

BATCHES, REPS, NBINS = 9, 10, 100
R_BELOW, R_ABOVE, R_SOLID, L = 0.75, 1.1, 1.5, 6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def run(name, q, box, rc):
    n = len(q)
    qd = torch.from_numpy(q).cuda()
    nl = NeighListGPU(rc, *box, dtype=torch.float32, full_list=True, minimum_image=True)
    nl.Initialize(n)
    nl.MakeNeighList(qd, n)
    hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
    sizes = torch.empty(n, dtype=torch.int32, device="cuda")
    summary = torch.empty(4, dtype=torch.int64, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    nl.set_steinhardt(L, R_SOLID, w=False)
    nl.steinhardt(qd)
    nl.solid_bonds(qd, 0.7, out=count)
    print(f"{name}: n {n}, entries {nl.number_of_pairs()}, solid bonds at l = {L}, threshold 0.7: mean {float(count.double().mean()):.3f} of "
          f"{float(nl.steinhardt_qlm()[1].double().mean()):.2f} neighbours", flush=True)
    for r in (R_BELOW, R_ABOVE):
        lab, sz, sm = nl.clusters(qd, r, sizes=sizes, summary=summary)
        s, c = cluster.size_distribution(lab)
        sm = sm.tolist()
        assert sm[0] == n and (s * c).sum() == n and c.sum() == sm[1] and s[-1] == sm[2] and int(sz[sm[3]]) == sm[2]
        assert (sm[2] > n // 2) == (r == R_ABOVE)
        print(f"{name}: r_max {r:g}: {sm[1]} clusters, the largest {sm[2]} (label {sm[3]}), singletons {int(c[0]) if s[0] == 1 else 0}", flush=True)
    calls = {}
    for r in (R_BELOW, R_ABOVE):
        calls[f"histogram to {r:g}"] = lambda r=r: nl.pair_histogram(qd, r, NBINS, out=hist)
        calls[f"clusters at {r:g}"] = lambda r=r: nl.clusters(qd, r, sizes=sizes, summary=summary)
        calls[f"clusters at {r:g}, labels alone"] = lambda r=r: nl.clusters(qd, r, sizes=False, summary=False)
    calls[f"histogram to {R_SOLID:g}"] = lambda: nl.pair_histogram(qd, R_SOLID, NBINS, out=hist)
    calls[f"solid bonds, l = {L}"] = lambda: nl.solid_bonds(qd, 0.7, out=count)
    ms = {k: [] for k in calls}
    for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
        for k, fn in calls.items():
            t = timed(fn)
            if batch:
                ms[k].append(t)
    for k, v in ms.items():
        v = np.array(v)
        r = f"{R_SOLID:g}" if k.startswith("solid") else k.split(",")[0].split()[-1]
        y = np.median(ms[f"histogram to {r}"])
        print(f"{name}, {k:32s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), {np.median(v) / y:.2f} x histogram to {r}", flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
    for name, rc in (("cfg2", 3.3), ("tight", 1.6)):
        if not only or name in only:
            run(name, q, box, rc)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What does the common neighbour analysis cost against the Steinhardt call on the same list?  fp32,
N = 2^20: 64^3 cells of fcc at density 1 (a = 4^(1/3), neighbour distance 1.1225), every atom displaced by a Gaussian of 3 % of
the neighbour distance per axis, in cell order; one handle and one full list per workload:
  cfg2    rc = 3.3 (about 150 entries a row): the walk dominates
  tight   rc = 1.8 (18 entries a row): what is behind the walk dominates
nl_cna fixed (r_max = the conventional fcc cut-off, 12 candidates) and adaptive (r_max = 1.7: 18 candidates, the 12 nearest
analysed), with and without the counts; the yardsticks on the same list in the same process: nl_steinhardt(l = 6, average = 0) to
the fixed cut-off and nl_pair_histogram to it.  The tool first asserts that more than 99 % of the atoms come out fcc.
Interleaved batches: every batch times each of the calls REPS times back to back between two events; the figure is the median
over the batches of the batch's mean, with the spread of the batches beside it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, cna  # noqa: E402

BATCHES, REPS, NBINS, CELLS = 7, 10, 100, 64
A = 4.0 ** (1.0 / 3.0)
R_FIXED, R_ADAPTIVE = cna.default_r_max("fcc", A), 1.7


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
    nl.set_steinhardt(6, R_FIXED, w=False)
    o = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
    counts = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    summary = torch.empty(6, dtype=torch.int64, device="cuda")
    for adaptive, r in ((False, R_FIXED), (True, R_ADAPTIVE)):
        t, c, s = nl.cna(qd, r, adaptive=adaptive, counts=counts, summary=summary)
        torch.cuda.synchronize()
        print(f"{name}: n {n}, entries {nl.number_of_pairs()}, {'adaptive' if adaptive else 'fixed'} r_max {r:.4f}: candidates mean "
              f"{float(c[:, 0].double().mean()):.2f} max {int(c[:, 0].max())}, summary {s.tolist()}", flush=True)
        assert int(s[cna.FCC]) > 0.99 * n and int(s[:5].sum()) == n
    calls = {
        "histogram": lambda: nl.pair_histogram(qd, R_FIXED, NBINS, out=hist),
        "steinhardt l = 6, average off": lambda: nl.steinhardt(qd, average=False, out=o),
        "cna fixed": lambda: nl.cna(qd, R_FIXED, adaptive=False, summary=summary),
        "cna fixed, counts": lambda: nl.cna(qd, R_FIXED, adaptive=False, counts=counts, summary=summary),
        "cna adaptive": lambda: nl.cna(qd, R_ADAPTIVE, adaptive=True, summary=summary),
        "cna adaptive, counts": lambda: nl.cna(qd, R_ADAPTIVE, adaptive=True, counts=counts, summary=summary),
    }
    ms = {k: [] for k in calls}
    for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
        for k, fn in calls.items():
            t = timed(fn)
            if batch:
                ms[k].append(t)
    ref = np.median(ms["steinhardt l = 6, average off"])
    for k, v in ms.items():
        v = np.array(v)
        print(f"{name}, {k:30s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), {np.median(v) / ref:.2f} x steinhardt, "
              f"{np.median(v) / np.median(ms['histogram']):.2f} x histogram", flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    p, box = cna.lattice("fcc", CELLS, A)
    rng = np.random.default_rng(1)
    p = (p + 0.25 * A + rng.normal(0.0, 0.03 * A * np.sqrt(0.5), size=p.shape)) % box
    q = np.zeros((len(p), 4), dtype=np.float32)
    q[:, :3] = p
    box = tuple(float(b) for b in box)
    q[:, :3] = np.minimum(q[:, :3], np.nextafter(np.float32(box[0]), np.float32(0)))
    for name, rc in (("cfg2", 3.3), ("tight", 1.8)):
        if not only or name in only:
            run(name, q, box, rc)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The three consumers on local-index slab lists next to the whole-box calls: cfg 2 (N = 2^20, rho = 1,
rc = 3.3, fp32, 30 z layers) cut into 2 and into 8 slabs on one device, half and full lists.  Per slab a build under
nl_set_local_ids (owned rows first, then the two ghost layers), then nl_lj_forces, nl_lj_virial and nl_pair_histogram (256
bins up to rc) on it; the whole-box calls of the same three on a whole build of the same handle kind.  Calls alternate, REPS
times each; medians, in ms.  A decomposition reports the slowest slab (what a step waits for when every rank has a device)
and the sum over its slabs (the work the cuts add: a crossing pair is evaluated on both sides).
--whole: the whole-box calls only, one line per list kind -- what an A/B of two builds of the library compares (NL_HIP_LIB
picks the library; one from before nl_set_local_ids loads too)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--whole", action="store_true")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
if args.whole:  # (the switch is not used: a library without it is timed all the same)
    for name in ("nl_set_local_ids", "nl_get_local_ids"):
        _lib.PROTOTYPES.pop(name, None)
from md_neighbor_list_amd import NeighListGPU, inputs, slab  # noqa: E402

REPS, RC, RCF, NBINS = args.reps, 3.3, 3.0, 256
q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
n = len(q)
qd = torch.from_numpy(q).cuda()
mz = int(box[2] / RC)
iz = slab.z_layer(qd, box, RC)


def timed(calls):
    """{name: (median, min, max) ms} of the calls, alternated REPS times behind one warm-up turn."""
    ms = {name: [] for name, _ in calls}
    for rep in range(REPS + 1):
        for name, f in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if rep:
                ms[name].append(a.elapsed_time(b))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def consumers(nl, qs, rows):
    f = torch.empty((rows, 4), dtype=torch.float32, device="cuda")
    w = torch.empty(8, dtype=torch.float64, device="cuda")
    h = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
    res = timed([("forces", lambda: nl.lj_forces(qs, 1.0, 1.0, rc_force=RCF, out=f)),
                 ("virial", lambda: nl.lj_virial(qs, 1.0, 1.0, rc_force=RCF, out=w)),
                 ("histogram", lambda: nl.pair_histogram(qs, RC, NBINS, out=h))])
    return res, w.cpu().numpy(), h.cpu().numpy() // (REPS + 1)


NAMES = ("forces", "virial", "histogram")
for full in (False, True):
    kind = "full" if full else "half"
    nl = NeighListGPU(RC, *box, dtype=torch.float32, full_list=full)
    nl.Initialize(n)
    nl.MakeNeighList(qd, n)
    whole, w_all, h_all = consumers(nl, qd, n)
    print(f"whole box, {kind} list, {int(h_all.sum())} pairs below {RC}: " +
          "  ".join(f"{k} {whole[k][0]:.3f} ms (min {whole[k][1]:.3f}, max {whole[k][2]:.3f})" for k in NAMES), flush=True)
    if args.whole:
        continue
    nl.set_local_ids(True)
    for world in (2, 8):
        worst, total = dict.fromkeys(NAMES, 0.0), dict.fromkeys(NAMES, 0.0)
        w_sum, h_sum, ghosts = np.zeros(8), np.zeros(NBINS, dtype=np.int64), 0
        for z_lo, z_hi in slab.split_layers(mz, world):
            own = torch.nonzero((iz >= z_lo) & (iz < z_hi)).flatten()
            glo = torch.nonzero(iz == (z_lo - 1) % mz).flatten()
            ghi = torch.nonzero(iz == z_hi % mz).flatten()
            qs = qd[torch.cat([own, glo, ghi])].contiguous()
            nl.MakeNeighListSlab(qs, None, len(own), z_lo, z_hi)
            res, w, h = consumers(nl, qs, len(own))
            for k in NAMES:
                worst[k], total[k] = max(worst[k], res[k][0]), total[k] + res[k][0]
            w_sum, h_sum, ghosts = w_sum + w, h_sum + h, ghosts + len(glo) + len(ghi)
        assert np.array_equal(h_sum, h_all) and w_sum[7] == w_all[7], "the slabs do not add up to the whole box"
        print(f"  {world} slabs ({ghosts} ghosts in all): " +
              "  ".join(f"{k} slowest {worst[k]:.3f} sum {total[k]:.3f} ({total[k] / whole[k][0]:.2f} x whole)" for k in NAMES), flush=True)

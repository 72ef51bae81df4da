#!/usr/bin/env python3
"""Build time per periodic-axes mask (nl_set_periodic_axes) at BASELINE config 2 (N = 1 M, rho = 1.0) and config 3
(rho = 0.5), fp32, rc = 3.3: 0 = open box (the reference's rule), 7 = fully periodic, 3 = xy (a film), 4 = z.
One handle per mask on the same positions; the masks take turns batch by batch (interleaved), each batch `reps`
asynchronous builds between two HIP events; reported: the median over batches, in ms per build.

usage: tools/time_periodic_axes.py [--masks 0,7,3,4] [--batches 9] [--reps 20] [--cfgs 2,3]
(masks 0 and 7 go through nl_set_periodic, so that the same script times a library without nl_set_periodic_axes)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402

CFGS = {2: (1 << 20, 1.0), 3: (1 << 20, 0.5)}
NAMES = {0: "open", 7: "xyz", 3: "xy", 4: "z", 1: "x", 2: "y", 5: "xz", 6: "yz"}


def handle(mask, box, n):
    nl = NeighListGPU(3.3, *box, dtype=torch.float32)
    if mask == 7:
        nl.set_periodic(True)
    elif mask:
        nl.set_periodic(axes=NAMES[mask])
    nl.Initialize(n)
    return nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", default="0,7,3,4")
    ap.add_argument("--cfgs", default="2,3")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    masks = [int(m) for m in args.masks.split(",")]
    print(f"ms per build, median of {args.batches} batches of {args.reps} (HIP events), masks interleaved; fp32, rc 3.3")
    for cfg in (int(c) for c in args.cfgs.split(",")):
        n, rho = CFGS[cfg]
        q, box = inputs.uniform_box(n, rho, np.float32)
        qd = torch.from_numpy(q).cuda()
        nls = {m: handle(m, box, n) for m in masks}
        for nl in nls.values():  # warm-up: allocations, list growth, path choice
            for _ in range(3):
                nl.MakeNeighList(qd, n)
        times = {m: [] for m in masks}
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.batches):
            for m in masks:
                nl = nls[m]
                ev[0].record()
                for _ in range(args.reps):
                    nl.MakeNeighList(qd, n, sync=False)
                ev[1].record()
                nl.synchronize()
                times[m].append(ev[0].elapsed_time(ev[1]) / args.reps)
        base = float(np.median(times[masks[0]]))
        for m in masks:
            t = np.array(times[m])
            print(f"cfg {cfg} (N={n}, rho={rho}) mask {m} ({NAMES[m]:4s}): {np.median(t):.4f} ms  "
                  f"[min {t.min():.4f}, max {t.max():.4f}]  x{np.median(t) / base:.3f} of mask {masks[0]}  "
                  f"pairs {nls[m].half_number_of_pairs()}")
        del nls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

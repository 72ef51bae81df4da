#!/usr/bin/env python3
"""Device time of one nl_update_list: skipped (no particle past skin / 2) and performed (one particle pushed past it and
back, alternately), against a plain nl_make_list on the same positions.  Uniform random box, rho = 1, rc = 3.3 (the
cut-off including the skin), skin 0.4, fp32 -- BASELINE config 2 at the default N.  HIP events around `reps` enqueued
calls on one stream; no host sync inside the window.

usage: tools/time_update.py [--n 1048576] [--reps 200] [--graph]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--graph", action="store_true")
    args = ap.parse_args()
    import numpy as np

    q, box = inputs.uniform_box(args.n, 1.0, np.float32)
    qd = torch.from_numpy(q).cuda()
    nl = NeighListGPU(3.3, *box, dtype=torch.float32)
    nl.Initialize(args.n)
    nl.set_graph(args.graph)
    nl.set_skin(0.4)
    nl.update(qd, sync=True)
    u0 = nl.update_stats()
    skipped = timed(lambda: nl.update(qd), args.reps)
    u1 = nl.update_stats()
    assert u1[1] == u0[1], "a skipped update built"
    flip = [0]

    def moved():
        flip[0] ^= 1
        qd[0, 0] += 0.5 if flip[0] else -0.5  # (one tiny kernel: part of the time below)
        nl.update(qd)

    bump = timed(lambda: qd[0, 0].add_(0.0), args.reps)
    performed = timed(moved, args.reps)
    u2 = nl.update_stats()
    assert u2[1] - u1[1] == u2[0] - u1[0], "a performed update did not build"
    nl.synchronize()
    make = timed(lambda: nl.MakeNeighList(qd, args.n, sync=False), args.reps)
    nl.synchronize()
    print(f"N={args.n} graph={int(args.graph)} skipped update {skipped:.1f} us, performed update {performed - bump:.1f} us "
          f"(position bump {bump:.1f} us subtracted), nl_make_list {make:.1f} us; pairs {nl.half_number_of_pairs()}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Build time of triclinic boxes (nl_set_box) at BASELINE config 2 (N = 1 M, rho = 1.0) and config 3 (rho = 0.5), fp32,
rc = 3.3, against the orthogonal box: mask 0 (open), mask 7 orthogonal, mask 7 with xy = 0.2 L (mesh 30^3 at cfg 2),
xy = 0.5 L (27 x 30 x 30), xy = xz = yz = 0.5 L (26 x 27 x 30), and the hexagonal slab (mask 3, xy = 0.5 L).
The same particles in every box: lambda = q / L of the orthogonal box, placed at lambda_a a + lambda_b b + lambda_c c.
One handle per case; the cases take turns batch by batch (interleaved), each batch `reps` asynchronous builds between two
HIP events; reported: the median over batches, in ms per build.  Then the cost of nl_set_box plus the build it forces,
against a plain synchronous build: the same mesh (xy moved by 1e-3 L) and a changed one (xy 0.2 L <-> 0.5 L).

usage: tools/time_box.py [--cfgs 2,3] [--batches 9] [--reps 20] [--cases ...] [--out profiles/r10_triclinic.txt]
With a library without nl_set_box (NL_HIP_LIB of an older build) only the orthogonal cases run.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402

CFGS = {2: (1 << 20, 1.0), 3: (1 << 20, 0.5)}
# name: (mask, tilt as fractions of L)
CASES = {
    "open": (0, (0.0, 0.0, 0.0)),
    "orth7": (7, (0.0, 0.0, 0.0)),
    "xy0.2": (7, (0.2, 0.0, 0.0)),
    "xy0.5": (7, (0.5, 0.0, 0.0)),
    "all0.5": (7, (0.5, 0.5, 0.5)),
    "slab3": (3, (0.5, 0.0, 0.0)),
}


def place(q, box, tilt):
    L = np.array(box, dtype=np.float64)
    lam = q[:, :3].astype(np.float64) / L
    xy, xz, yz = tilt
    p = np.stack([lam[:, 0] * L[0] + lam[:, 1] * xy + lam[:, 2] * xz, lam[:, 1] * L[1] + lam[:, 2] * yz, lam[:, 2] * L[2]], axis=1)
    out = q.copy()
    out[:, :3] = p.astype(q.dtype)
    return out


def handle(mask, box, tilt, n):
    nl = NeighListGPU(3.3, *box, dtype=torch.float32)
    if mask == 7:
        nl.set_periodic(True)
    elif mask:
        nl.set_periodic(axes="xy")
    if any(tilt):
        nl.set_box(*box, *tilt)
    nl.Initialize(n)
    return nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="2,3")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--setbox-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    has_box = hasattr(NeighListGPU, "set_box")
    try:
        from md_neighbor_list_amd import _lib

        has_box = has_box and hasattr(_lib.load(), "nl_set_box")
    except Exception:
        has_box = False
    cases = [c for c in args.cases.split(",") if has_box or not any(CASES[c][1])]
    say(f"ms per build, median of {args.batches} batches of {args.reps} (HIP events), cases interleaved; fp32, rc 3.3, "
        f"lib {os.environ.get('NL_HIP_LIB', 'in-tree')}")
    for cfg in (int(c) for c in args.cfgs.split(",")):
        n, rho = CFGS[cfg]
        q, box = inputs.uniform_box(n, rho, np.float32)
        qds, nls = {}, {}
        for c in cases:
            mask, f = CASES[c]
            tilt = tuple(v * box[0] for v in f)
            qds[c] = torch.from_numpy(place(q, box, tilt)).cuda()
            nls[c] = handle(mask, box, tilt, n)
        for c in cases:  # warm-up: allocations, list growth, path choice
            for _ in range(3):
                nls[c].MakeNeighList(qds[c], n)
        times = {c: [] for c in cases}
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.batches):
            for c in cases:
                nl = nls[c]
                ev[0].record()
                for _ in range(args.reps):
                    nl.MakeNeighList(qds[c], n, sync=False)
                ev[1].record()
                nl.synchronize()
                times[c].append(ev[0].elapsed_time(ev[1]) / args.reps)
        ref = "orth7" if "orth7" in times else cases[0]
        base = float(np.median(times[ref]))
        base_cells = np.prod(nls[ref].mesh_size)
        for c in cases:
            t = np.array(times[c])
            m = nls[c].mesh_size
            cells = m[0] * m[1] * m[2]
            say(f"cfg {cfg} (N={n}, rho={rho}) {c:7s} mask {CASES[c][0]} mesh {m[0]}x{m[1]}x{m[2]}: {np.median(t):.4f} ms  "
                f"[min {t.min():.4f}, max {t.max():.4f}]  x{np.median(t) / base:.3f} of orth7  "
                f"candidates x{base_cells / cells:.2f}  pairs {nls[c].half_number_of_pairs()}")
        if has_box and cfg == 2:
            # nl_set_box + the forced synchronous build, against a plain synchronous build
            L = box[0]
            nl = handle(7, box, (0.2 * L, 0.0, 0.0), n)
            qa, qb = qds.get("xy0.2"), qds.get("xy0.5")
            if qa is not None and qb is not None:
                for _ in range(3):
                    nl.MakeNeighList(qa, n)

                def timed(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(args.setbox_reps):
                        fn(k)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / args.setbox_reps * 1e3

                plain = timed(lambda k: nl.MakeNeighList(qa, n))
                same = timed(lambda k: (nl.set_box(*box, (0.2 + 1e-3 * (k & 1)) * L, 0.0, 0.0), nl.MakeNeighList(qa, n)))
                nl.set_box(*box, 0.2 * L, 0.0, 0.0)
                changed = timed(lambda k: (nl.set_box(*box, (0.5 if k & 1 else 0.2) * L, 0.0, 0.0),
                                           nl.MakeNeighList(qb if k & 1 else qa, n)))
                say(f"cfg 2 host wall per synchronous build ({args.setbox_reps} reps): plain {plain:.3f} ms, "
                    f"nl_set_box (same mesh) + build {same:.3f} ms, nl_set_box (mesh 30^3 <-> 27x30x30) + build {changed:.3f} ms")
        del nls, qds
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of a type table (nl_set_type_cutoffs) at BASELINE config 2 (N = 1 M, rho = 1.0) and config 3 (rho = 0.5), fp32,
rc = 3.3.  Types: seeded 80:20 A:B; rc_AA = 3.3, rc_AB = 2.64, rc_BB = 2.904 (Kob-Andersen's ratios at rc = 3.3 sigma_AA).
Reported, median over interleaved batches of `reps` asynchronous calls between two HIP events:
  1. a build without the table, with it, and with the types plus the exclusion table of tools/time_exclusions.py;
  2. a device-to-device copy of the unfiltered list (torch copy_, the same number of int32 entries), for scale;
  3. nl_set_type_cutoffs (synchronous, wall clock);
  4. a skipped nl_update_list with the table set;
  5. typed Lennard-Jones on the typed list against untyped Lennard-Jones on the plain list (half lists).
The stage's own device time comes from `rocprofv3 --kernel-trace --stats` over `--stage-only` (k_type_count, the row scan,
k_type_compact); `--stats FILE` prints those kernels' medians from its results database (<name>_results.db).

usage: tools/time_type_cutoffs.py [--cfgs 2,3] [--batches 9] [--reps 20] [--stage-only] [--stats types_results.db]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402
from tools.time_exclusions import CFGS, table, timed  # noqa: E402

RC = 3.3
RCM = np.array([[3.3, 2.64], [2.64, 2.904]])
EPS = np.array([[1.0, 1.5], [1.5, 0.5]])
SIG = np.array([[1.0, 0.8], [0.8, 0.88]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="2,3")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-only", action="store_true", help="builds with the tables only (for a rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="print the k_type_* / k_excl_* / scan rows of a rocprofv3 results database")
    args = ap.parse_args()
    if args.stats:
        import sqlite3

        db = sqlite3.connect(args.stats)
        rows = db.execute("select name, duration from kernels where name like '%k_type%' or name like '%k_excl_c%' "
                          "or name like '%k_scan_chained%' or name like '%k_lj%'").fetchall()
        for name in sorted({r[0] for r in rows}):
            d = [r[1] for r in rows if r[0] == name]
            print(f"  {name[:90]:90s} calls {len(d)}  median {np.median(d) / 1e3:.1f} us  min {min(d) / 1e3:.1f} us")
        return
    print(f"ms, median of {args.batches} batches of {args.reps} (HIP events), interleaved; fp32, rc {RC}")
    for cfg in (int(c) for c in args.cfgs.split(",")):
        n, rho = CFGS[cfg]
        q, box = inputs.uniform_box(n, rho, np.float32)
        qd = torch.from_numpy(q).cuda()
        types = (np.random.default_rng(8020).uniform(size=n) < 0.2).astype(np.int32)
        td = torch.from_numpy(types).cuda()
        plain, typed, both = (NeighListGPU(RC, *box) for _ in range(3))
        for nl in (plain, typed, both):
            nl.Initialize(n)
        plain.MakeNeighList(qd, n)
        pairs = table(plain)
        total = plain.half_number_of_pairs()
        setup = []
        for _ in range(5):
            t0 = time.perf_counter()
            typed.set_type_cutoffs(td, RCM)
            setup.append((time.perf_counter() - t0) * 1e3)
        both.set_exclusions(pairs, n)
        both.set_type_cutoffs(td, RCM)
        for _ in range(3):
            for nl in (plain, typed, both):
                nl.MakeNeighList(qd, n)
        kept, kept_both = typed.half_number_of_pairs(), both.half_number_of_pairs()
        if args.stage_only:
            for _ in range(args.batches * args.reps):
                typed.MakeNeighList(qd, n, sync=False)
            typed.synchronize()
            for _ in range(args.batches * args.reps):
                both.MakeNeighList(qd, n, sync=False)
            both.synchronize()
            print(f"cfg {cfg}: {args.batches * args.reps} builds with types, then as many with types + exclusions; "
                  f"{total} -> {kept} / {kept_both} pairs")
            continue
        src = torch.empty(total, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        upd = NeighListGPU(RC, *box)
        upd.Initialize(n)
        upd.set_skin(0.3)
        upd.set_type_cutoffs(td, RCM)
        upd.update(qd, sync=True)
        typed.set_lj_type_params(EPS, SIG, np.minimum(2.5 * SIG, RCM))
        f = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        t = {"plain": [], "typed": [], "both": [], "copy": [], "skip": [], "lj": [], "lj_typed": []}
        for _ in range(args.batches):
            t["plain"].append(timed(lambda: plain.MakeNeighList(qd, n, sync=False), args.reps, plain.synchronize))
            t["typed"].append(timed(lambda: typed.MakeNeighList(qd, n, sync=False), args.reps, typed.synchronize))
            t["both"].append(timed(lambda: both.MakeNeighList(qd, n, sync=False), args.reps, both.synchronize))
            t["copy"].append(timed(lambda: dst.copy_(src), args.reps, torch.cuda.synchronize))
            t["skip"].append(timed(lambda: upd.update(qd), args.reps, upd.synchronize))
            t["lj"].append(timed(lambda: plain.lj_forces(qd, 1.0, 1.0, 2.5, out=f), args.reps, torch.cuda.synchronize))
            t["lj_typed"].append(timed(lambda: typed.lj_forces_typed(qd, out=f), args.reps, torch.cuda.synchronize))
        b0, s0 = upd.update_stats()
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"cfg {cfg} (N={n}, rho={rho}): {total} half pairs unfiltered; types keep {kept} "
              f"({100.0 * kept / total:.1f} %), types + {len(pairs)} excluded pairs keep {kept_both}")
        print(f"  build without table      {med['plain']:.4f} ms  [min {min(t['plain']):.4f}]")
        print(f"  build with types         {med['typed']:.4f} ms  [min {min(t['typed']):.4f}]  +{med['typed'] - med['plain']:.4f} ms")
        print(f"  build types + exclusions {med['both']:.4f} ms  [min {min(t['both']):.4f}]  +{med['both'] - med['plain']:.4f} ms")
        print(f"  D2D copy of the list     {med['copy']:.4f} ms  ({4 * total / 1e6:.0f} MB each way)")
        print(f"  stage (difference) / copy = {(med['typed'] - med['plain']) / med['copy']:.2f}")
        print(f"  nl_set_type_cutoffs      {np.median(setup):.2f} ms wall  [min {min(setup):.2f}]")
        print(f"  skipped update with types {med['skip'] * 1e3:.1f} us  (updates {b0}, builds {s0})")
        print(f"  LJ untyped (plain list)  {med['lj']:.4f} ms;  LJ typed (typed list) {med['lj_typed']:.4f} ms")
        del plain, typed, both, upd, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

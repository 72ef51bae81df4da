#!/usr/bin/env python3
"""Cost of an exclusion table (nl_set_exclusions) at BASELINE config 2 (N = 1 M, rho = 1.0) and config 3 (rho = 0.5),
fp32, rc = 3.3.  The table: each particle's first two listed partners (about 2 M pairs, every one of them in the list).
Reported, median over interleaved batches of `reps` asynchronous calls between two HIP events:
  1. a build without and with the table (two handles, same positions);
  2. a device-to-device copy of the unfiltered list (torch copy_, the same number of int32 entries), timed in the same process;
  3. nl_set_exclusions (synchronous, wall clock);
  4. a skipped nl_update_list with the table set.
The stage's own device time comes from `rocprofv3 --kernel-trace --stats` over `--stage-only` (k_excl_count, the row scan,
k_excl_compact); `--stats FILE` prints those kernels' medians from its results database (<name>_results.db).

usage: tools/time_exclusions.py [--cfgs 2,3] [--batches 9] [--reps 20] [--stage-only] [--stats excl_results.db]
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


def table(nl):
    kp = nl.key_pointer().long()
    sl = nl.sorted_list().long()
    cnt = nl.half_number_of_partners().long()
    rows = torch.arange(len(cnt), device=kp.device)
    out = []
    for k in (0, 1):
        m = cnt > k
        out.append(torch.stack([rows[m], sl[kp[:-1][m] + k]], dim=1))
    return torch.cat(out).to(torch.int32)


def timed(fn, reps, sync):
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    sync()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="2,3")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-only", action="store_true", help="builds with the table only (for a rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="print the k_excl_* / scan rows of a rocprofv3 kernel_stats.csv")
    args = ap.parse_args()
    if args.stats:
        import sqlite3

        db = sqlite3.connect(args.stats)
        rows = db.execute("select name, duration from kernels where name like '%k_excl%' or name like '%k_scan_chained%'").fetchall()
        for name in sorted({r[0] for r in rows}):
            d = [r[1] for r in rows if r[0] == name]
            print(f"  {name[:90]:90s} calls {len(d)}  median {np.median(d) / 1e3:.1f} us  min {min(d) / 1e3:.1f} us")
        return
    print(f"ms, median of {args.batches} batches of {args.reps} (HIP events), interleaved; fp32, rc 3.3")
    for cfg in (int(c) for c in args.cfgs.split(",")):
        n, rho = CFGS[cfg]
        q, box = inputs.uniform_box(n, rho, np.float32)
        qd = torch.from_numpy(q).cuda()
        plain, excl = NeighListGPU(3.3, *box), NeighListGPU(3.3, *box)
        plain.Initialize(n)
        excl.Initialize(n)
        plain.MakeNeighList(qd, n)
        pairs = table(plain)
        total = plain.half_number_of_pairs()
        setup = []
        for _ in range(5):
            t0 = time.perf_counter()
            excl.set_exclusions(pairs, n)
            setup.append((time.perf_counter() - t0) * 1e3)
        for _ in range(3):
            excl.MakeNeighList(qd, n)
            plain.MakeNeighList(qd, n)
        kept = excl.half_number_of_pairs()
        if args.stage_only:
            for _ in range(args.batches * args.reps):
                excl.MakeNeighList(qd, n, sync=False)
            excl.synchronize()
            print(f"cfg {cfg}: {args.batches * args.reps} builds with the table, {total - kept} pairs dropped")
            continue
        src = torch.empty(total, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        upd = NeighListGPU(3.3, *box)
        upd.Initialize(n)
        upd.set_skin(0.3)
        upd.set_exclusions(pairs, n)
        upd.update(qd, sync=True)
        t = {"plain": [], "excl": [], "copy": [], "skip": []}
        for _ in range(args.batches):
            t["plain"].append(timed(lambda: plain.MakeNeighList(qd, n, sync=False), args.reps, plain.synchronize))
            t["excl"].append(timed(lambda: excl.MakeNeighList(qd, n, sync=False), args.reps, excl.synchronize))
            t["copy"].append(timed(lambda: dst.copy_(src), args.reps, torch.cuda.synchronize))
            t["skip"].append(timed(lambda: upd.update(qd), args.reps, upd.synchronize))
        b0, s0 = upd.update_stats()
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"cfg {cfg} (N={n}, rho={rho}): {total} half pairs, table {len(pairs)} pairs, {total - kept} dropped")
        print(f"  build without table  {med['plain']:.4f} ms  [min {min(t['plain']):.4f}]")
        print(f"  build with table     {med['excl']:.4f} ms  [min {min(t['excl']):.4f}]  +{med['excl'] - med['plain']:.4f} ms")
        print(f"  D2D copy of the list {med['copy']:.4f} ms  ({4 * total / 1e6:.0f} MB each way, "
              f"{8 * total / med['copy'] / 1e6:.0f} GB/s read+write)")
        print(f"  stage (difference) / copy = {(med['excl'] - med['plain']) / med['copy']:.2f}")
        print(f"  nl_set_exclusions    {np.median(setup):.2f} ms wall  [min {min(setup):.2f}]")
        print(f"  skipped update with table {med['skip'] * 1e3:.1f} us  (updates {b0}, builds {s0})")
        del plain, excl, upd, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

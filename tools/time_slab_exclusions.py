#!/usr/bin/env python3
"""Cost of the exclusion stage with a table keyed by global id (nl_set_exclusions_global), fp32, rc = 3.3, rho = 1.0.
The sibling of tools/time_exclusions.py: the same table (each row's first two listed partners, every pair in the list),
the same interleaved batches of asynchronous builds between two HIP events.

  cfg2   BASELINE config 2 (N = 1 M) as ONE slab holding every layer, so that every table kind can be timed on one list:
           whole build            no table | input-row table | global table (ids are rows: the row-indexed pass)
           the same with a gid array (ids = rows, explicit)   no table | global table (the pass loads gid[row])
           the same with NL_GID_IN_W                          no table | global table (the pass loads the positions' w)
         The yardstick of the id-indexed pass is the row-indexed pass on the same list: ratio of the two stage costs.
  cfg4   one interior slab of the 8-slab decomposition of BASELINE config 4 (N = 32 M; ids in w, n_ids = N):
           no table | global table.  (An input-row table refuses a slab build.)

usage: tools/time_slab_exclusions.py [--cases cfg2,cfg4] [--batches 9] [--reps 10]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs, slab  # noqa: E402

RC = 3.3


def first_partners(nl, row_ids):
    """[E, 2] int32: every row's first two listed partners, as (row id, partner id)."""
    kp, sl, cnt = nl.key_pointer().long(), nl.sorted_list().long(), nl.half_number_of_partners().long()
    out = []
    for k in (0, 1):
        m = cnt > k
        out.append(torch.stack([row_ids[m], sl[kp[:-1][m] + k]], dim=1))
    return torch.cat(out).to(torch.int32)


def timed(fn, reps, sync):
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    sync()
    return ev[0].elapsed_time(ev[1]) / reps


def interleaved(fns, batches, reps):
    """{name: (median, min, max)} of `batches` rounds over all of fns, `reps` asynchronous calls each."""
    t = {k: [] for k in fns}
    for k, (fn, sync) in fns.items():  # warm-up, growth
        fn()
        sync()
    for _ in range(batches):
        for k, (fn, sync) in fns.items():
            t[k].append(timed(fn, reps, sync))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def report(res, pairs_of):
    for k, (med, lo, hi) in res.items():
        print(f"  {k:44s} {med:8.4f} ms  [min {lo:.4f}, max {hi:.4f}]  {pairs_of.get(k, '')}", flush=True)


def cfg2(args):
    n = 1 << 20
    q, box = inputs.uniform_box(n, 1.0, np.float32)
    mz = int(box[2] / RC)
    qd = torch.from_numpy(q).cuda()
    gid = torch.arange(n, dtype=torch.int32, device="cuda")
    qw = qd.clone()
    qw[:, 3] = gid.view(torch.float32)
    h = {k: NeighListGPU(RC, *box) for k in ("plain", "rows", "glob", "gid", "gid_glob", "w", "w_glob")}
    for nl in h.values():
        nl.Initialize(n)
    h["plain"].MakeNeighList(qd, n)
    total = h["plain"].half_number_of_pairs()
    pairs = first_partners(h["plain"], torch.arange(n, device="cuda"))
    h["rows"].set_exclusions(pairs, n)
    setup = []
    for k in ("glob", "gid_glob", "w_glob"):
        t0 = time.perf_counter()
        h[k].set_exclusions_global(pairs, n)
        setup.append((time.perf_counter() - t0) * 1e3)
    fns = {
        "whole, no table": (lambda: h["plain"].MakeNeighList(qd, n, sync=False), h["plain"].synchronize),
        "whole, input-row table": (lambda: h["rows"].MakeNeighList(qd, n, sync=False), h["rows"].synchronize),
        "whole, global table (row-indexed)": (lambda: h["glob"].MakeNeighList(qd, n, sync=False), h["glob"].synchronize),
        "gid array, no table": (lambda: h["gid"].MakeNeighListSlab(qd, gid, n, 0, mz, sync=False), h["gid"].synchronize),
        "gid array, global table (gid[row])": (lambda: h["gid_glob"].MakeNeighListSlab(qd, gid, n, 0, mz, sync=False), h["gid_glob"].synchronize),
        "ids in w, no table": (lambda: h["w"].MakeNeighListSlab(qw, "w", n, 0, mz, sync=False), h["w"].synchronize),
        "ids in w, global table (q[row].w)": (lambda: h["w_glob"].MakeNeighListSlab(qw, "w", n, 0, mz, sync=False), h["w_glob"].synchronize),
    }
    res = interleaved(fns, args.batches, args.reps)
    kept = {k: h[k].half_number_of_pairs() for k in ("rows", "glob", "gid_glob", "w_glob")}
    assert len(set(kept.values())) == 1, kept
    print(f"cfg 2 as one slab (N = {n}): {total} half pairs, table {len(pairs)} pairs, {total - kept['rows']} dropped; "
          f"nl_set_exclusions_global {np.median(setup):.2f} ms wall")
    report(res, {})
    m = {k: v[0] for k, v in res.items()}
    row = m["whole, input-row table"] - m["whole, no table"]
    print(f"  stage, row-indexed (input-row table)  +{row:.4f} ms")
    print(f"  stage, row-indexed (global table)     +{m['whole, global table (row-indexed)'] - m['whole, no table']:.4f} ms")
    for name, a, b in (("gid[row]", "gid array, global table (gid[row])", "gid array, no table"),
                       ("q[row].w", "ids in w, global table (q[row].w)", "ids in w, no table")):
        d = m[a] - m[b]
        print(f"  stage, id-indexed ({name})          +{d:.4f} ms   ratio to the row-indexed stage {d / row:.3f}")
    spread = max((v[2] - v[1]) / v[0] for v in res.values())
    print(f"  largest run-to-run spread of a line (max - min) / median: {100 * spread:.2f} %")


def cfg4(args):
    n = 1 << 25
    q, box = inputs.uniform_box(n, 1.0, np.float32)
    mz = int(box[2] / RC)
    z_lo, z_hi = slab.split_layers(mz, 8)[3]
    iz = slab.z_layer(torch.from_numpy(q), box, RC).numpy()
    own = np.flatnonzero((iz >= z_lo) & (iz < z_hi))
    glo, ghi = np.flatnonzero(iz == (z_lo - 1) % mz), np.flatnonzero(iz == z_hi % mz)
    idx = np.concatenate([own, glo, ghi])
    qa = torch.from_numpy(q[idx]).cuda()
    ids = torch.from_numpy(idx.astype(np.int32)).cuda()
    qa[:, 3] = ids.view(torch.float32)
    del q, iz
    per = (2.0 / 3.0) * np.pi * RC ** 3
    h = {k: NeighListGPU(RC, *box) for k in ("plain", "glob")}
    for nl in h.values():
        nl.Initialize(len(idx))
        nl.set_capacity(int(len(own) * per * 1.3) + 64 * len(own) + 4096)
    h["plain"].MakeNeighListSlab(qa, "w", len(own), z_lo, z_hi)
    total = h["plain"].half_number_of_pairs()
    pairs = first_partners(h["plain"], ids[: len(own)].long())
    t0 = time.perf_counter()
    h["glob"].set_exclusions_global(pairs, n)
    setup = (time.perf_counter() - t0) * 1e3
    fns = {
        "slab, no table": (lambda: h["plain"].MakeNeighListSlab(qa, "w", len(own), z_lo, z_hi, sync=False), h["plain"].synchronize),
        "slab, global table (q[row].w)": (lambda: h["glob"].MakeNeighListSlab(qa, "w", len(own), z_lo, z_hi, sync=False), h["glob"].synchronize),
    }
    res = interleaved(fns, args.batches, args.reps)
    kept = h["glob"].half_number_of_pairs()
    print(f"cfg 4, slab 3 of 8 (layers [{z_lo}, {z_hi}) of {mz}; {len(own)} owned + {len(glo)} + {len(ghi)} ghosts, n_ids = {n}: "
          f"{4 * (n + 1) / 1e6:.0f} MB of offsets): {total} half pairs, table {len(pairs)} pairs, {total - kept} dropped; "
          f"nl_set_exclusions_global {setup:.1f} ms wall")
    report(res, {})
    m = {k: v[0] for k, v in res.items()}
    print(f"  stage, id-indexed (q[row].w)  +{m['slab, global table (q[row].w)'] - m['slab, no table']:.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cfg2,cfg4")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    print(f"ms, median of {args.batches} interleaved batches of {args.reps} asynchronous builds (HIP events); fp32, rc {RC}")
    for case in args.cases.split(","):
        {"cfg2": cfg2, "cfg4": cfg4}[case](args)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the image stage (nl_set_pair_images) and of nl_pair_vectors at BASELINE config 2 (N = 1 M, rho = 1.0) and
config 3 (rho = 0.5), fp32, rc = 3.3, minimum image on every axis (mask 7), half list.
Reported, median over interleaved batches of `reps` asynchronous calls between two HIP events:
  1. a build with the flag off and with it on (two handles, same positions): the stage is the difference;
  2. yardstick 1: a device-to-device copy of the list (torch copy_, the same number of int32 entries), in the same process;
  3. yardstick 2: a build with an exclusion table (each particle's first two listed partners) on the same list: its stage
     (k_excl_count, the row scan, k_excl_compact) is the bar the image stage must stay under;
  4. nl_pair_vectors, against the 16 bytes per entry it must write over the HBM peak (8.0 TB/s, MI355X_MICROARCH.md);
  5. a skipped nl_update_list with the flag on and with it off;
  6. the stage and nl_pair_vectors again on the same particles shifted by +1 along x, so that 1 % of them lie outside the
     box and are wrapped (k_pair_images then gathers the partner's code for every entry), with the ids as given (random
     in space) and in cell order (nl_resort): the gather is what the order of the ids changes.
The kernels' own device times come from `rocprofv3 --kernel-trace --stats` over `--stage-only`; `--stats FILE` prints their
medians from its results database (<name>_results.db).

usage: tools/time_pair_images.py [--cfgs 2,3] [--batches 9] [--reps 20] [--stage-only] [--stats images_results.db]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402
from tools.time_exclusions import table, timed  # noqa: E402

CFGS = {2: (1 << 20, 1.0), 3: (1 << 20, 0.5)}
HBM_PEAK = 8.0e12  # bytes/s (MI355X_MICROARCH.md)
KERNELS = ("k_image_codes", "k_pair_images", "k_zero_images", "k_pair_vectors", "k_excl_count", "k_excl_compact", "k_scan_chained")


def handle(box, n, images=False, skin=None):
    nl = NeighListGPU(3.3, *box, minimum_image=True)
    nl.Initialize(n)
    if images:
        nl.set_pair_images(True)
    if skin is not None:
        nl.set_skin(skin)
    return nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="2,3")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stage-only", action="store_true", help="builds with the flag / the table and pair_vectors only (for a rocprofv3 run)")
    ap.add_argument("--stats", default=None, help="print the kernels of both stages from a rocprofv3 results database")
    args = ap.parse_args()
    if args.stats:
        import sqlite3

        db = sqlite3.connect(args.stats)
        where = " or ".join(f"name like '%{k}%'" for k in KERNELS)
        rows = db.execute(f"select name, duration from kernels where {where}").fetchall()
        for name in sorted({r[0] for r in rows}):
            d = [r[1] for r in rows if r[0] == name]
            print(f"  {name[:90]:90s} calls {len(d)}  median {np.median(d) / 1e3:.1f} us  min {min(d) / 1e3:.1f} us")
        # k_pair_images in launch order: per cfg, the builds of the input as given, then of the wrapped input
        d = [r[0] for r in db.execute("select duration from kernels where name like '%k_pair_images%' order by start").fetchall()]
        print("  k_pair_images in launch order, medians of consecutive tenths (us): " +
              " ".join(f"{np.median(c) / 1e3:.0f}" for c in np.array_split(np.array(d), 10) if len(c)))
        return
    print(f"ms, median of {args.batches} batches of {args.reps} (HIP events), interleaved; fp32, rc 3.3, mask 7, half list")
    for cfg in (int(c) for c in args.cfgs.split(",")):
        n, rho = CFGS[cfg]
        q, box = inputs.uniform_box(n, rho, np.float32)
        qd = torch.from_numpy(q).cuda()
        plain, img, excl = handle(box, n), handle(box, n, images=True), handle(box, n)
        plain.MakeNeighList(qd, n)
        excl.set_exclusions(table(plain), n)
        total = plain.half_number_of_pairs()
        for _ in range(3):
            for nl in (plain, img, excl):
                nl.MakeNeighList(qd, n)
        assert img.half_number_of_pairs() == total
        nonzero = float((img.pair_images() != 0).any(dim=1).float().mean())
        out = torch.empty((total + 65536, 4), dtype=torch.float32, device="cuda")  # (the shifted input: a few pairs more or fewer)
        img.pair_vectors(qd, out=out)
        if args.stage_only:
            for _ in range(args.batches * args.reps):
                img.MakeNeighList(qd, n, sync=False)
            img.synchronize()
            for _ in range(args.batches * args.reps):
                excl.MakeNeighList(qd, n, sync=False)
            excl.synchronize()
            for _ in range(args.batches * args.reps):
                img.pair_vectors(qd, out=out)
            torch.cuda.synchronize()
            qs = qd.clone()
            qs[:, 0] += 1.0  # (1 % of the particles wrapped: every entry gathers; these launches follow the first in the trace)
            img.MakeNeighList(qs, n)
            for _ in range(args.batches * args.reps):
                img.MakeNeighList(qs, n, sync=False)
            img.synchronize()
            print(f"cfg {cfg}: {args.batches * args.reps} builds with images, with the table, pair_vectors calls, "
                  f"builds with images of wrapped input; {total} entries")
            continue
        src = torch.empty(total, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        upd_on, upd_off = handle(box, n, images=True, skin=0.3), handle(box, n, skin=0.3)
        upd_on.update(qd, sync=True)
        upd_off.update(qd, sync=True)
        t = {k: [] for k in ("plain", "img", "excl", "copy", "vec", "skip_on", "skip_off")}
        for _ in range(args.batches):
            t["plain"].append(timed(lambda: plain.MakeNeighList(qd, n, sync=False), args.reps, plain.synchronize))
            t["img"].append(timed(lambda: img.MakeNeighList(qd, n, sync=False), args.reps, img.synchronize))
            t["excl"].append(timed(lambda: excl.MakeNeighList(qd, n, sync=False), args.reps, excl.synchronize))
            t["copy"].append(timed(lambda: dst.copy_(src), args.reps, torch.cuda.synchronize))
            t["vec"].append(timed(lambda: img.pair_vectors(qd, out=out), args.reps, torch.cuda.synchronize))
            t["skip_on"].append(timed(lambda: upd_on.update(qd), args.reps, upd_on.synchronize))
            t["skip_off"].append(timed(lambda: upd_off.update(qd), args.reps, upd_off.synchronize))
        assert upd_on.update_stats()[1] == 1 and upd_off.update_stats()[1] == 1  # every timed update skipped
        med = {k: float(np.median(v)) for k, v in t.items()}
        stage, bar = med["img"] - med["plain"], med["excl"] - med["plain"]
        floor = 16.0 * total / HBM_PEAK * 1e3
        print(f"cfg {cfg} (N={n}, rho={rho}): {total} entries, {100 * nonzero:.1f} % with a nonzero image")
        print(f"  build, flag off        {med['plain']:.4f} ms  [min {min(t['plain']):.4f}, max {max(t['plain']):.4f}]")
        print(f"  build, flag on         {med['img']:.4f} ms  [min {min(t['img']):.4f}]  stage +{stage:.4f} ms")
        print(f"  build, exclusion table {med['excl']:.4f} ms  [min {min(t['excl']):.4f}]  stage +{bar:.4f} ms")
        print(f"  D2D copy of the list   {med['copy']:.4f} ms  ({4 * total / 1e6:.0f} MB each way, "
              f"{8 * total / med['copy'] / 1e6:.0f} GB/s read+write)")
        print(f"  image stage / copy = {stage / med['copy']:.2f}   image stage / exclusion stage = {stage / bar:.2f}")
        print(f"  nl_pair_vectors        {med['vec']:.4f} ms  [min {min(t['vec']):.4f}]  write floor {floor:.4f} ms "
              f"(16 B an entry at 8.0 TB/s): {100 * floor / med['vec']:.0f} % of that bound")
        print(f"  skipped update, flag on {med['skip_on'] * 1e3:.1f} us, flag off {med['skip_off'] * 1e3:.1f} us")
        # the same particles, 1 % of them wrapped; then with their ids in cell order
        qs = qd.clone()
        qs[:, 0] += 1.0
        for label in ("shifted +1 in x, ids as given", "shifted +1 in x, ids in cell order"):
            plain.MakeNeighList(qs, n)
            if "cell order" in label:
                plain.resort(qs)
            for _ in range(3):
                plain.MakeNeighList(qs, n)
                img.MakeNeighList(qs, n)
            nz = float((img.pair_images() != 0).any(dim=1).float().mean())
            u = {k: [] for k in ("plain", "img", "vec")}
            for _ in range(args.batches):
                u["plain"].append(timed(lambda: plain.MakeNeighList(qs, n, sync=False), args.reps, plain.synchronize))
                u["img"].append(timed(lambda: img.MakeNeighList(qs, n, sync=False), args.reps, img.synchronize))
                u["vec"].append(timed(lambda: img.pair_vectors(qs, out=out), args.reps, torch.cuda.synchronize))
            m = {k: float(np.median(v)) for k, v in u.items()}
            print(f"  {label}: {img.half_number_of_pairs()} entries, {100 * nz:.1f} % nonzero; build {m['plain']:.4f} -> {m['img']:.4f} ms, stage +{m['img'] - m['plain']:.4f} ms "
                  f"({(m['img'] - m['plain']) / med['copy']:.2f} x copy); nl_pair_vectors {m['vec']:.4f} ms")
        del plain, img, excl, upd_on, upd_off, src, dst, out, qs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""nl_pair_histogram against nl_lj_virial on the same list: cfg 2 (N = 2^20, rho = 1, rc = 3.3, fp32),
half and full builds, ids in random and in cell order.  The virial walks the same rows and gathers the same positions with
more arithmetic and no LDS atomics, so it is the yardstick.  Per list: the untyped histogram at 256 and at 4096 bins
(counters in LDS), and on a second handle with a table of two types (every rc_ab = rc: the same pairs) the typed one at
3 x 256 counters (LDS) and 3 x 2048 (beyond NL_HIST_LDS_COUNTERS: every entry added to the device tensor).  Calls alternate,
REPS times each; medians, in ms."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402

REPS, RC = 9, 3.3
q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
n = len(q)
qd0 = torch.from_numpy(q).cuda()
nl0 = NeighListGPU(RC, *box, dtype=torch.float32)
nl0.Initialize(n)
nl0.MakeNeighList(qd0, n)
qs = qd0[nl0.sorted_state()[1].long()].contiguous()  # the same particles in cell order
types = torch.from_numpy(np.random.default_rng(1).integers(0, 2, size=n).astype(np.int32)).cuda()
torch.cuda.synchronize()


def timed(calls):
    """{name: median ms} of the calls, alternated REPS times behind one warm-up turn."""
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


for order, qd in (("random", qd0), ("cell", qs)):
    for full in (False, True):
        nl = NeighListGPU(RC, *box, dtype=torch.float32, full_list=full)
        nl.Initialize(n)
        nl.MakeNeighList(qd, n)
        ty = NeighListGPU(RC, *box, dtype=torch.float32, full_list=full)
        ty.Initialize(n)
        ty.set_type_cutoffs(types, [[RC, RC], [RC, RC]])
        ty.MakeNeighList(qd, n)
        w = torch.empty(8, dtype=torch.float64, device="cuda")
        h256, h4096 = (torch.zeros(b, dtype=torch.int64, device="cuda") for b in (256, 4096))
        t256, t2048 = (torch.zeros((3, b), dtype=torch.int64, device="cuda") for b in (256, 2048))
        res = timed([
            ("virial", lambda: nl.lj_virial(qd, 1.0, 1.0, rc_force=3.0, out=w)),
            ("hist 256", lambda: nl.pair_histogram(qd, RC, 256, out=h256)),
            ("hist 4096", lambda: nl.pair_histogram(qd, RC, 4096, out=h4096)),
            ("virial (table)", lambda: ty.lj_virial(qd, 1.0, 1.0, rc_force=3.0, out=w)),
            ("typed 3x256 lds", lambda: ty.pair_histogram(qd, RC, 256, typed=True, out=t256)),
            ("typed 3x2048 global", lambda: ty.pair_histogram(qd, RC, 2048, typed=True, out=t2048)),
        ])
        pairs = int(h256.sum()) // (REPS + 1)
        assert pairs == int(h4096.sum()) // (REPS + 1) == int(t256.sum()) // (REPS + 1) == int(t2048.sum()) // (REPS + 1)
        assert torch.equal(t2048.view(3, 256, 8).sum(dim=2), t256)
        v = res["virial"][0]
        print(f"{order:6s} order, {'full' if full else 'half'} list, {pairs} pairs below {RC}:", flush=True)
        for name, (med, lo, hi) in res.items():
            print(f"    {name:20s} {med:7.3f} ms  (min {lo:.3f}, max {hi:.3f})  {med / v:5.2f} x virial", flush=True)

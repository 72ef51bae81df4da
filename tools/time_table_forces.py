#!/usr/bin/env python3
"""What does a tabulated pair potential cost against Lennard-Jones in closed form?  cfg 2 (N = 2^20,
rho = 1, rc = 3.3, fp32), half and full list, on one handle and one list per list kind: nl_lj_forces against nl_table_forces
with the table staged in LDS and with the table read from global memory (set under NL_TABLE_LDS=0), and the same three for
the totals (nl_lj_virial, nl_table_virial).  The table is a Morse potential at 1024 knots (16 KiB in fp32), r_max = rc_force =
3.0.  Interleaved batches: every batch times each of the six calls REPS times back to back between two events; the figure
is the median over the batches of the batch's mean, with the spread of the batches beside it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs, pair_table  # noqa: E402

BATCHES, REPS, NK, R_MIN, R_MAX = 9, 10, 1024, 1e-3, 3.0


def morse(De=1.0, a=1.5, r0=1.125):
    return (lambda r: De * ((1.0 - np.exp(-a * (r - r0))) ** 2 - 1.0),
            lambda r: 2.0 * De * a * (1.0 - np.exp(-a * (r - r0))) * np.exp(-a * (r - r0)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
    F, U = pair_table.sample(*morse(), R_MIN, R_MAX, NK)
    qd = torch.from_numpy(q).cuda()
    for full in (False, True):
        nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=full)
        nl.Initialize(len(q))
        nl.MakeNeighList(qd, len(q))
        f = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
        w = torch.empty(8, dtype=torch.float64, device="cuda")

        def table(lds):
            if lds:
                os.environ.pop("NL_TABLE_LDS", None)
            else:
                os.environ["NL_TABLE_LDS"] = "0"
            nl.set_pair_table(F, U, R_MIN, R_MAX)

        calls = {
            "lj forces": (None, lambda: nl.lj_forces(qd, 1.0, 1.0, rc_force=R_MAX, out=f)),
            "table forces, LDS": (True, lambda: nl.table_forces(qd, out=f)),
            "table forces, global": (False, lambda: nl.table_forces(qd, out=f)),
            "lj virial": (None, lambda: nl.lj_virial(qd, 1.0, 1.0, rc_force=R_MAX, out=w)),
            "table virial, LDS": (True, lambda: nl.table_virial(qd, out=w)),
            "table virial, global": (False, lambda: nl.table_virial(qd, out=w)),
        }
        ms = {name: [] for name in calls}
        sums = {}
        for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
            for name, (lds, fn) in calls.items():
                if lds is not None:
                    table(lds)
                t = timed(fn)
                if batch:
                    ms[name].append(t)
                sums[name] = float(f[:, :3].abs().sum()) if "forces" in name else float(w[7])
        for name, v in ms.items():
            v = np.array(v)
            ref = np.median(ms["lj forces" if "forces" in name else "lj virial"])
            print(f"{'full' if full else 'half'} list, {name:22s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), "
                  f"{np.median(v) / ref:.3f} x lj; {'|f| checksum' if 'forces' in name else 'pairs'} {sums[name]:.6e}", flush=True)


if __name__ == "__main__":
    main()

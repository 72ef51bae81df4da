#!/usr/bin/env python3
"""What does an embedded-atom potential cost against its pair part alone?  cfg 2 (N = 2^20, rho = 1,
rc = 3.3, fp32), half and full list, on one handle and one list per list kind: nl_table_forces / nl_table_virial (the
yardstick, the pair table in LDS) against nl_eam_forces / nl_eam_virial with the tables staged in LDS and with the tables read
from global memory (set under NL_TABLE_LDS=0).  The pair part is a Morse potential at 1024 knots, the density f = exp(-2 (r -
1.125)) at 1024 knots (together 32 KiB in fp32), the embedding -2 sqrt(rho + 1) + 0.005 rho^2 at 1024 knots, r_max = 3.0 for
both.  Interleaved batches: every batch times each of the six calls REPS times back to back between two events; the figure is
the median over the batches of the batch's mean, with the spread of the batches beside it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, eam, inputs, pair_table  # noqa: E402

BATCHES, REPS, NK, R_MIN, R_MAX, RHO_MAX = 9, 10, 1024, 1e-3, 3.0, 400.0


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
    tabs = eam.sample(lambda r: np.exp(-2.0 * (r - 1.125)), lambda r: -2.0 * np.exp(-2.0 * (r - 1.125)),
                      lambda x: -2.0 * np.sqrt(x + 1.0) + 0.005 * x * x, lambda x: -1.0 / np.sqrt(x + 1.0) + 0.01 * x,
                      R_MIN, R_MAX, NK, RHO_MAX, NK)
    qd = torch.from_numpy(q).cuda()
    for full in (False, True):
        nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=full)
        nl.Initialize(len(q))
        nl.MakeNeighList(qd, len(q))
        f = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
        w = torch.empty(8, dtype=torch.float64, device="cuda")
        os.environ.pop("NL_TABLE_LDS", None)
        nl.set_pair_table(F, U, R_MIN, R_MAX)

        def tables(lds):
            if lds:
                os.environ.pop("NL_TABLE_LDS", None)
            else:
                os.environ["NL_TABLE_LDS"] = "0"
            nl.set_eam(tabs[0], tabs[1], R_MIN, R_MAX, tabs[2], tabs[3], RHO_MAX)
            assert nl.eam()["lds_forces"] == lds and nl.eam()["lds_density"] == lds

        calls = {
            "table forces": (None, lambda: nl.table_forces(qd, out=f)),
            "eam forces, LDS": (True, lambda: nl.eam_forces(qd, out=f)),
            "eam forces, global": (False, lambda: nl.eam_forces(qd, out=f)),
            "table virial": (None, lambda: nl.table_virial(qd, out=w)),
            "eam virial, LDS": (True, lambda: nl.eam_virial(qd, out=w)),
            "eam virial, global": (False, lambda: nl.eam_virial(qd, out=w)),
        }
        ms = {name: [] for name in calls}
        sums = {}
        for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
            for name, (lds, fn) in calls.items():
                if lds is not None:
                    tables(lds)
                t = timed(fn)
                if batch:
                    ms[name].append(t)
                sums[name] = float(f[:, :3].abs().sum()) if "forces" in name else float(w[7])
        rho = nl.eam_density()[0]
        print(f"{'full' if full else 'half'} list: rho {float(rho.min()):.3f} .. {float(rho.max()):.3f}, finite forces "
              f"{bool(torch.isfinite(f).all())}", flush=True)
        for name, v in ms.items():
            v = np.array(v)
            ref = np.median(ms["table forces" if "forces" in name else "table virial"])
            print(f"{'full' if full else 'half'} list, {name:20s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), "
                  f"{np.median(v) / ref:.3f} x table; {'|f| checksum' if 'forces' in name else 'pairs'} {sums[name]:.6e}", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What does the DPD pair term cost against the charge term?  cfg 2 (N = 2^20, rho = 1, rc = 3.3, fp32),
half and full list, on one handle and one list per list kind: nl_coul_forces / nl_coul_virial (the yardstick: the same walk
with one gathered array, both tables in LDS) against nl_dpd_forces / nl_dpd_virial with the pair table, the weight table and
the slot parameters staged in LDS and with all read from global memory (the DPD state set under NL_TABLE_LDS=0).  The pair
table is a Morse potential at 1024 knots to r_max = 3.0, the charge table the real-space Ewald term (alpha = 0.9) and the
weight table w = 1 - r / r_max, both at 1024 knots to the same r_max: 32 KiB of LDS either way.  Charges +-1 at random,
velocities normal, gamma = 4.5, kT = 1.
Each list kind twice: the particles in the random order of the input, and re-sorted into cell order (nl_resort of positions,
charges and velocities, then a rebuild), where the partners of a row share cache lines.
Interleaved batches: every batch times each call REPS times back to back between two events; the figure is the median over
the batches of the batch's mean, with the spread of the batches beside it.
--yardstick: the charge calls alone, for a library of the parent commit (NL_HIP_LIB), which has no nl_*dpd* symbols."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import _lib  # noqa: E402

YARDSTICK = "--yardstick" in sys.argv
if YARDSTICK:
    for name in [k for k in _lib.PROTOTYPES if "dpd" in k]:
        del _lib.PROTOTYPES[name]
from md_neighbor_list_amd import NeighListGPU, coulomb, dpd, inputs, pair_table  # noqa: E402

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
    rng = np.random.default_rng(3)
    F, U = pair_table.sample(*morse(), R_MIN, R_MAX, NK)
    K, Cc = coulomb.ewald_real(0.9, R_MIN, R_MAX, NK)
    A = dpd.weight(R_MIN, R_MAX, NK)
    q0 = torch.from_numpy(q).cuda()
    chg0 = torch.from_numpy(np.where(rng.random(len(q)) < 0.5, 1.0, -1.0).astype(np.float32)).cuda()
    v0 = torch.from_numpy(rng.normal(size=(len(q), 3)).astype(np.float32)).cuda()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    for full, resorted in ((False, False), (True, False), (False, True), (True, True)):
        qd, chg, vd = q0.clone(), chg0.clone(), v0.clone()
        nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=full)
        nl.Initialize(len(q))
        nl.MakeNeighList(qd, len(q))
        if resorted:
            nl.resort(qd, chg, vd)
            nl.MakeNeighList(qd, len(q))
        f = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
        w = torch.empty(8, dtype=torch.float64, device="cuda")
        os.environ.pop("NL_TABLE_LDS", None)
        nl.set_pair_table(F, U, R_MIN, R_MAX)
        nl.set_coulomb_table(K, Cc, R_MIN, R_MAX)
        nl.set_charges(chg)

        def state(lds):
            if lds:
                os.environ.pop("NL_TABLE_LDS", None)
            else:
                os.environ["NL_TABLE_LDS"] = "0"
            nl.set_dpd(A, 4.5, dpd.sigma_for(4.5, 1.0), R_MIN, R_MAX, 0.01, 12345)
            assert nl.dpd_info()["lds"] == lds

        calls = {"coul forces": (None, lambda: nl.coul_forces(qd, out=f)), "coul virial": (None, lambda: nl.coul_virial(qd, out=w))}
        if not YARDSTICK:
            calls.update({
                "dpd forces, LDS": (True, lambda: nl.dpd_forces(qd, vd, step, out=f)),
                "dpd forces, global": (False, lambda: nl.dpd_forces(qd, vd, step, out=f)),
                "dpd virial, LDS": (True, lambda: nl.dpd_virial(qd, vd, step, out=w)),
                "dpd virial, global": (False, lambda: nl.dpd_virial(qd, vd, step, out=w)),
            })
        ms = {name: [] for name in calls}
        sums = {}
        for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
            for name, (lds, fn) in calls.items():
                if lds is not None:
                    state(lds)
                t = timed(fn)
                if batch:
                    ms[name].append(t)
                sums[name] = float(f[:, :3].abs().sum()) if "forces" in name else float(w[7])
        for name, v in ms.items():
            v = np.array(v)
            ref = np.median(ms["coul forces" if "forces" in name else "coul virial"])
            print(f"{'full' if full else 'half'} list, {'cell order' if resorted else 'input order'}, {name:20s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), "
                  f"{np.median(v) / ref:.3f} x coul; {'|f| checksum' if 'forces' in name else 'pairs'} {sums[name]:.6e}", flush=True)


if __name__ == "__main__":
    main()

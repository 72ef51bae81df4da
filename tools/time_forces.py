#!/usr/bin/env python3
"""Which list kind serves a force loop better?  cfg 2: build + nl_lj_forces for the half list
(pair once + atomics) and the full list (gather, no atomics), and beside them nl_lj_virial on the same list (the totals:
a read pass for both list kinds), alternating with the forces, in two rounds.  --pbc: the minimum-image list of a periodic box, where the
consumer folds every separation (the open box, the default here, never enters lj_image's fold).  --tilt: the same
box with tilts of a quarter of its edges, the triclinic instances of the consumer."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, inputs  # noqa: E402

TILT = "--tilt" in sys.argv[1:]
PBC = TILT or "--pbc" in sys.argv[1:]
q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
KW = dict(minimum_image=PBC, tilt=(0.25 * box[0], -0.25 * box[0], 0.25 * box[1]) if TILT else None)
qd0 = torch.from_numpy(q).cuda()
nl0 = NeighListGPU(3.3, *box, dtype=torch.float32, **KW)
nl0.Initialize(len(q))
nl0.MakeNeighList(qd0, len(q))
qs = qd0[nl0.sorted_state()[1].long()].contiguous()  # the same particles in cell order (SORT_FREQ, section 8 f2)
torch.cuda.synchronize()
for rnd in range(2):
    for order, qd, full in (("random", qd0, False), ("random", qd0, True), ("cell", qs, False), ("cell", qs, True)):
        nl = NeighListGPU(3.3, *box, dtype=torch.float32, full_list=full, **KW)
        nl.Initialize(len(q))
        nl.MakeNeighList(qd, len(q))
        w = torch.empty(8, dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        tb, tf, tv = [], [], []
        for rep in range(6):
            ev[0].record()
            nl.MakeNeighList(qd, len(q), sync=False)
            ev[1].record()
            f = nl.lj_forces(qd, 1.0, 1.0, rc_force=3.0)
            ev[2].record()
            nl.lj_virial(qd, 1.0, 1.0, rc_force=3.0, out=w)
            ev[3].record()
            torch.cuda.synchronize()
            tb.append(ev[0].elapsed_time(ev[1])), tf.append(ev[1].elapsed_time(ev[2])), tv.append(ev[2].elapsed_time(ev[3]))
        print(f"round {rnd}: {'tilted ' if TILT else 'periodic ' if PBC else ''}{order:6s} order, {'full' if full else 'half'} list: "
              f"build {min(tb[1:]):.3f} ms, forces {min(tf[1:]):.3f} ms, virial {min(tv[1:]):.3f} ms, "
              f"build + forces {min(tb[1:]) + min(tf[1:]):.3f} ms; |f| checksum {float(f[:, :3].abs().sum()):.6e}, "
              f"tr W {float(w[:3].sum()):.9e}, U {float(w[6]):.9e}, pairs {int(w[7])}", flush=True)

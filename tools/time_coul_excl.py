#!/usr/bin/env python3
"""What does the excluded-pair term cost?  cfg 2 (N = 2^20, rho = 1, rc = 3.3, fp32) with the chain
topology: particles 4 m .. 4 m + 3 form a chain with its 1-2 and 1-3 pairs excluded (rows of 2 and 3 ids, 2.5 N entries).  The
chains join particles of the uniform random box wherever they are, so the table runs from 1e-3 to the box diagonal; what is
timed is the walk, not the physics.  nl_coul_excl_forces (add = 0) and nl_coul_excl_virial, the table in LDS and read from
global memory (set under NL_TABLE_LDS=0), the particles in the random order of the input and re-sorted into cell order
(nl_resort of positions and charges, then a rebuild, which relabels the table) -- where chain mates are no longer neighbours
in memory.  The parent has no such call, so every time stands against two yardsticks:
  1. the same sum on the consumers' wave per row: a second build of the library with -DNL_COUL_EXCL_LANES=64
     (csrc/nl_coul_excl.inc), made by --build-yardstick into build/libnl_hip_wave_row.so and timed by --yardstick;
  2. the traffic floor of the walk -- positions 16 N, charges 4 N, offsets 4 N, ids 4 E, the row store 16 N (the totals: none)
     -- over the HBM rate of bench.py's roofline.
Interleaved batches: every batch times each call REPS times back to back between two events; the figure is the median over
the batches of the batch's mean, with the spread of the batches beside it.  Run the tool once plain and once with --yardstick
in the same visit and compare the lines."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD_LIB = os.path.join(ROOT, "build", "libnl_hip_wave_row.so")
YARDSTICK = "--yardstick" in sys.argv

if "--build-yardstick" in sys.argv:
    os.makedirs(os.path.dirname(YARD_LIB), exist_ok=True)
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()  # (the Makefile's)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-DNL_COUL_EXCL_LANES=64", "-shared", "-o", YARD_LIB,
                           os.path.join(ROOT, "md_neighbor_list_amd", "csrc", "nl_api.hip")])
    sys.exit(0)
if YARDSTICK:
    os.environ["NL_HIP_LIB"] = YARD_LIB

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from md_neighbor_list_amd import NeighListGPU, coulomb, inputs  # noqa: E402

BATCHES, REPS, NK, R_MIN = 9, 10, 1024, 1e-3
HBM_GBS = 8000.0  # HBM_PEAK_GBS of bench.py


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
    n = len(q)
    r_max = float(np.sqrt(3.0) * max(box)) * 1.01
    K, Cc = coulomb.ewald_excluded(0.9, R_MIN, r_max, NK)
    base = np.arange(0, n, 4, dtype=np.int32)
    pairs = np.concatenate([np.stack([base + a, base + b], axis=1) for a, b in ((0, 1), (1, 2), (2, 3), (0, 2), (1, 3))])
    entries = 2 * len(pairs)
    floor_ms = (16 * n + 4 * n + 4 * n + 4 * entries + 16 * n) / (HBM_GBS * 1e9) * 1e3
    q0 = torch.from_numpy(q).cuda()
    chg0 = torch.from_numpy(np.where(np.random.default_rng(3).random(n) < 0.5, 1.0, -1.0).astype(np.float32)).cuda()
    walk = "wave per row (yardstick)" if YARDSTICK else "8 lanes per row"
    for resorted in (False, True):
        qd, chg = q0.clone(), chg0.clone()
        nl = NeighListGPU(3.3, *box, dtype=torch.float32)
        nl.Initialize(n)
        nl.set_exclusions(pairs, n)
        nl.MakeNeighList(qd, n)
        if resorted:
            nl.resort(qd, chg)
            nl.MakeNeighList(qd, n)
        nl.set_charges(chg)
        f = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        w = torch.empty(8, dtype=torch.float64, device="cuda")

        def table(lds):
            if lds:
                os.environ.pop("NL_TABLE_LDS", None)
            else:
                os.environ["NL_TABLE_LDS"] = "0"
            nl.set_excluded_coulomb_table(K, Cc, R_MIN, r_max)
            assert nl.excluded_coulomb_table_info()["lds"] == lds

        calls = {
            "forces, LDS": (True, lambda: nl.coul_excl_forces(qd, out=f)),
            "forces, global": (False, lambda: nl.coul_excl_forces(qd, out=f)),
            "virial, LDS": (True, lambda: nl.coul_excl_virial(qd, out=w)),
            "virial, global": (False, lambda: nl.coul_excl_virial(qd, out=w)),
        }
        ms = {name: [] for name in calls}
        sums = {}
        for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
            for name, (lds, fn) in calls.items():
                table(lds)
                t = timed(fn)
                if batch:
                    ms[name].append(t)
                sums[name] = float(f[:, :3].abs().sum()) if "forces" in name else float(w[7])
        for name, v in ms.items():
            v = np.array(v)
            print(f"{walk}, {'cell order' if resorted else 'input order'}, {name:15s}: median {np.median(v) * 1e3:.1f} us (batches {v.min() * 1e3:.1f} .. "
                  f"{v.max() * 1e3:.1f}), {np.median(v) / floor_ms:.2f} x the traffic floor of {floor_ms * 1e3:.1f} us; "
                  f"{'|f| checksum' if 'forces' in name else 'pairs'} {sums[name]:.6e}", flush=True)


if __name__ == "__main__":
    main()

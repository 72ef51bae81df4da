#!/usr/bin/env python3
"""What do the Steinhardt order parameters cost against the other consumers of the same list?  fp32, N = 2^20
uniform particles at rho = 1, one handle and one full list per workload:
  cfg2    rc = 3.3 (about 150 entries a row), r_max = 1.5: about 14 of them are neighbours -- the walk dominates
  tight   rc = 1.6 (about 17 entries a row), r_max = 1.5: nearly every entry is a neighbour -- arithmetic and reductions dominate
The yardsticks run on the same list in the same process: nl_pair_histogram to r_max (the same walk, almost no arithmetic) and
nl_table_forces with a Morse table of 1024 knots (to 3.0 on cfg2, to 1.5 on tight).  nl_steinhardt: l = 6 and 12, average off
and on.  The tool first asserts that nothing is NaN.  Interleaved batches: every batch times each of the calls REPS times back to
back between two events; the figure is the median over the batches of the batch's mean, with the spread of the batches beside it.
--yardstick: the yardsticks alone, for a library of the parent commit (NL_HIP_LIB), which has no nl_steinhardt* symbols; run it
before and behind the full run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import _lib  # noqa: E402

YARDSTICK = "--yardstick" in sys.argv
if YARDSTICK:
    for name in [k for k in _lib.PROTOTYPES if "steinhardt" in k]:
        del _lib.PROTOTYPES[name]
from md_neighbor_list_amd import NeighListGPU, inputs, pair_table  # noqa: E402

BATCHES, REPS, NK, R_MAX, NBINS = 9, 10, 1024, 1.5, 100


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


def run(name, q, box, rc, table_to):
    qd = torch.from_numpy(q).cuda()
    nl = NeighListGPU(rc, *box, dtype=torch.float32, full_list=True)
    nl.Initialize(len(q))
    nl.MakeNeighList(qd, len(q))
    f = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
    o = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
    hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
    nl.set_pair_table(*pair_table.sample(*morse(), 1e-3, table_to, NK), 1e-3, table_to)
    calls = {"histogram": (None, lambda: nl.pair_histogram(qd, R_MAX, NBINS, out=hist)), "table forces": (None, lambda: nl.table_forces(qd, out=f))}
    nl.table_forces(qd, out=f)
    assert bool(torch.isfinite(f).all())
    if not YARDSTICK:
        for l in (6, 12):
            for avg in (False, True):
                calls[f"steinhardt l = {l:2d}, average {'on' if avg else 'off'}"] = (l, lambda avg=avg: nl.steinhardt(qd, average=avg, out=o))
            nl.set_steinhardt(l, R_MAX)
            nl.steinhardt(qd, average=True, out=o)
            nb = nl.steinhardt_qlm()[1].double()
            ok = nb > 0
            assert bool(torch.isfinite(o[ok]).all()) and bool(torch.isnan(o[~ok]).all())
            print(f"{name}: n {len(q)}, entries {nl.number_of_pairs()}, l {l}: neighbours within {R_MAX:g} mean {float(nb.mean()):.2f} max {int(nb.max())}, "
                  f"without any {int((~ok).sum())}; mean q_l {float(o[ok, 0].mean()):.4f}, averaged {float(o[ok, 2].mean()):.4f}", flush=True)
    ms = {k: [] for k in calls}
    at = None
    for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
        for k, (l, fn) in calls.items():
            if l is not None and l != at:
                nl.set_steinhardt(l, R_MAX)
                at = l
            t = timed(fn)
            if batch:
                ms[k].append(t)
    for k, v in ms.items():
        v = np.array(v)
        print(f"{name}, {k:32s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), {np.median(v) / np.median(ms['histogram']):.2f} x histogram, "
              f"{np.median(v) / np.median(ms['table forces']):.2f} x table forces", flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
    for name, rc, table_to in (("cfg2", 3.3, 3.0), ("tight", 1.6, 1.5)):
        if not only or name in only:
            run(name, q, box, rc, table_to)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What does a Stillinger-Weber potential cost against its pair part alone?  Two workloads in fp32, each on
one handle and one full list: nl_table_forces / nl_table_virial (the yardstick, the pair table in LDS) against nl_sw_forces /
nl_sw_virial with the tables staged in LDS and with the tables read from global memory (set under NL_TABLE_LDS=0).
  cfg2     N = 2^20, rho = 1, rc = 3.3: a Morse pair table to 3.0 at 1024 knots, g = exp(1.2 / (r - 3.2)) to r_max_3 = 1.8 at 1024
           knots (about 24 partners in range per centre)
  silicon  a diamond crystal of 51^3 cells (1 061 208 atoms) jittered by +-0.05 A, rc = 3.8, sw.silicon() at 1024 knots: 4
           partners in range, 6 triples per centre
The tool first asserts that nothing is NaN: no centre has more than 64 partners in range.  Interleaved batches: every batch
times each of the six calls REPS times back to back between two events; the figure is the median over the batches of the
batch's mean, with the spread of the batches beside it.
--yardstick: the table calls alone, for a library of the parent commit (NL_HIP_LIB), which has no nl_sw_* symbols."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import _lib  # noqa: E402

YARDSTICK = "--yardstick" in sys.argv
if YARDSTICK:
    for name in [k for k in _lib.PROTOTYPES if "_sw" in k]:
        del _lib.PROTOTYPES[name]
from md_neighbor_list_amd import NeighListGPU, inputs, pair_table, sw  # noqa: E402

BATCHES, REPS, NK = 9, 10, 1024


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


def cfg2():
    q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
    gf, dgf = sw.radial(1.2, 1.0, 3.2)
    return dict(q=q, box=box, rc=3.3, pair=pair_table.sample(*morse(), 1e-3, 3.0, NK), pair_range=(1e-3, 3.0),
                g=sw.sample(gf, dgf, 1e-3, 1.8, NK), g_range=(1e-3, 1.8), ang=sw.angular(2.0, 1.0, -1.0 / 3.0))


def silicon():
    si = sw.silicon()
    eps, sig, cells = si["epsilon"], si["sigma"], 51
    a0 = 4.0 * 2.0 ** (1.0 / 6.0) * sig / np.sqrt(3.0)
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]) / 4.0
    c = np.stack(np.meshgrid(*(np.arange(cells),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(7)
    p = ((c[:, None, :] + basis[None, :, :]).reshape(-1, 3) + 0.125) * a0
    q = np.zeros((len(p), 4), dtype=np.float32)
    q[:, :3] = p + rng.uniform(-0.05, 0.05, size=p.shape)
    r_min, r_max = 1.5, si["a"] * sig
    gf, dgf = sw.radial(si["gamma"], sig, si["a"])
    return dict(q=q, box=(cells * a0,) * 3, rc=3.8, pair=pair_table.sample(*sw.pair(si["A"], si["B"], si["p"], si["q"], eps, sig, si["a"]), r_min, r_max, NK),
                pair_range=(r_min, r_max), g=sw.sample(gf, dgf, r_min, r_max, NK), g_range=(r_min, r_max), ang=sw.angular(si["lam"], eps, si["cos0"]))


def run(name, w):
    q = w["q"]
    qd = torch.from_numpy(q).cuda()
    nl = NeighListGPU(w["rc"], *w["box"], dtype=torch.float32, full_list=True)
    nl.Initialize(len(q))
    nl.MakeNeighList(qd, len(q))
    f = torch.empty((len(q), 4), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    os.environ.pop("NL_TABLE_LDS", None)
    nl.set_pair_table(*w["pair"], *w["pair_range"])

    def tables(lds):
        if lds:
            os.environ.pop("NL_TABLE_LDS", None)
        else:
            os.environ["NL_TABLE_LDS"] = "0"
        nl.set_sw(*w["g"], *w["g_range"], *w["ang"])
        assert nl.sw()["lds"] == lds

    calls = {"table forces": (None, lambda: nl.table_forces(qd, out=f)), "table virial": (None, lambda: nl.table_virial(qd, out=out))}
    triples = None
    if not YARDSTICK:
        calls.update({
            "sw forces, LDS": (True, lambda: nl.sw_forces(qd, out=f)),
            "sw forces, global": (False, lambda: nl.sw_forces(qd, out=f)),
            "sw virial, LDS": (True, lambda: nl.sw_virial(qd, out=out)),
            "sw virial, global": (False, lambda: nl.sw_virial(qd, out=out)),
        })
        tables(True)
        nl.sw_forces(qd, out=f), nl.sw_virial(qd, out=out)
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(out).all()), "a centre with more than 64 partners in range"
        # the triples, from the list itself: the partners within r_max_3 of every row, m (m - 1) / 2 per centre
        kp, lst, _ = nl.full_csr()
        kp, lst = kp.long(), lst.long()
        rows = torch.repeat_interleave(torch.arange(len(q), device="cuda"), kp[1:] - kp[:-1])
        d = qd[rows, :3] - qd[lst, :3]
        L = torch.tensor(w["box"], dtype=torch.float32, device="cuda")
        d = d - torch.round(d / L) * L
        m = torch.bincount(rows[(d * d).sum(dim=1) < w["g_range"][1] ** 2], minlength=len(q)).double()
        triples = float((m * (m - 1) / 2).sum())
        print(f"{name}: n {len(q)}, entries {len(rows)}, partners in range mean {float(m.mean()):.2f} max {int(m.max())}, triples {triples:.4e}", flush=True)
    ms = {k: [] for k in calls}
    for batch in range(BATCHES + 1):  # (the first batch warms up and is dropped)
        for k, (lds, fn) in calls.items():
            if lds is not None:
                tables(lds)
            t = timed(fn)
            if batch:
                ms[k].append(t)
    for k, v in ms.items():
        v = np.array(v)
        ref = np.median(ms["table forces" if "forces" in k else "table virial"])
        rate = f", {triples / np.median(v) * 1e3:.4e} triples/s" if triples and k.startswith("sw") else ""
        print(f"{name}, {k:18s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), {np.median(v) / ref:.3f} x table{rate}", flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, make in (("cfg2", cfg2), ("silicon", silicon)):
        if not only or name in only:
            run(name, make())


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What does a Tersoff potential cost against a Stillinger-Weber potential on the same list?  Two workloads
in fp32, each on one handle and one full list: nl_sw_forces / nl_sw_virial (the yardstick, tools/time_sw_forces.py's tables, in
LDS) against nl_tersoff_forces / nl_tersoff_virial with the tables staged in LDS and with the tables read from global memory
(set under NL_TABLE_LDS=0).
  cfg2     N = 2^20, rho = 1, rc = 3.3: a Morse pair table to 3.0 at 1024 knots; Stillinger-Weber g to r_max_3 = 1.8; Tersoff u, q
           with f_C from 1.0 to 1.8, r_max_3 = 1.8, p = NULL (about 24 partners in range per centre)
  silicon  a diamond crystal of 51^3 cells (1 061 208 atoms), a = 5.432, jittered by +-0.05 A, rc = 3.8: sw.silicon() to 3.77 and
           tersoff.silicon() to 3.0 at 1024 knots: 4 partners in range
The tool first asserts that nothing is NaN.  Interleaved batches: every batch times each of the calls REPS times back to back
between two events; the figure is the median over the batches of the batch's mean, with the spread of the batches beside it.
--yardstick: the Stillinger-Weber calls alone, for a library of the parent commit (NL_HIP_LIB), which has no nl_tersoff_* symbols;
run it before and behind the full run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import _lib  # noqa: E402

YARDSTICK = "--yardstick" in sys.argv
if YARDSTICK:
    for name in [k for k in _lib.PROTOTYPES if "tersoff" in k]:
        del _lib.PROTOTYPES[name]
from md_neighbor_list_amd import NeighListGPU, inputs, pair_table, sw, tersoff  # noqa: E402

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


def tersoff_args(par, r_min, r_max):
    """The arguments of NeighListGPU.set_tersoff for a one-type LAMMPS parameter set, lambda_3 = 0."""
    u, U = tersoff.sample(*tersoff.attractive(par["B"], par["lam2"], par["R"], par["D"]), r_min, r_max, NK)
    q, Q = tersoff.sample(*tersoff.zeta_radial(0.0, par["R"], par["D"])[0], r_min, r_max, NK)
    return (u, U, q, Q, r_min, r_max) + tersoff.angular(par["gamma"], par["c"], par["d"], par["h"]) + tersoff.bond_order(par["beta"], par["n"])


def cfg2():
    q, box = inputs.uniform_box(1 << 20, 1.0, np.float32)
    gf, dgf = sw.radial(1.2, 1.0, 3.2)
    reduced = dict(B=1.0, lam2=1.2, R=1.4, D=0.4, gamma=0.02, c=1.0, d=0.15, h=0.0, beta=1.1, n=2.5)
    return dict(q=q, box=box, rc=3.3, pair=pair_table.sample(*morse(), 1e-3, 3.0, NK), pair_range=(1e-3, 3.0), r3=1.8,
                sw=sw.sample(gf, dgf, 1e-3, 1.8, NK) + (1e-3, 1.8) + sw.angular(2.0, 1.0, -1.0 / 3.0), tersoff=tersoff_args(reduced, 1e-3, 1.8))


def silicon():
    si, ts = sw.silicon(), tersoff.silicon()
    eps, sig, cells, a0 = si["epsilon"], si["sigma"], 51, 5.432
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]) / 4.0
    c = np.stack(np.meshgrid(*(np.arange(cells),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(7)
    p = ((c[:, None, :] + basis[None, :, :]).reshape(-1, 3) + 0.125) * a0
    q = np.zeros((len(p), 4), dtype=np.float32)
    q[:, :3] = p + rng.uniform(-0.05, 0.05, size=p.shape)
    r_min, r_max = 1.5, si["a"] * sig
    gf, dgf = sw.radial(si["gamma"], sig, si["a"])
    # one pair table under both: Tersoff's repulsive part on the Stillinger-Weber range (it is 0 from 3.0 on)
    return dict(q=q, box=(cells * a0,) * 3, rc=3.8, pair=pair_table.sample(*tersoff.repulsive(ts["A"], ts["lam1"], ts["R"], ts["D"]), r_min, r_max, NK),
                pair_range=(r_min, r_max), r3=ts["R"] + ts["D"], sw=sw.sample(gf, dgf, r_min, r_max, NK) + (r_min, r_max) + sw.angular(si["lam"], eps, si["cos0"]),
                tersoff=tersoff_args(ts, r_min, ts["R"] + ts["D"]))


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
    nl.set_sw(*w["sw"])
    assert nl.sw()["lds"]

    def tables(lds):
        if lds:
            os.environ.pop("NL_TABLE_LDS", None)
        else:
            os.environ["NL_TABLE_LDS"] = "0"
        nl.set_tersoff(*w["tersoff"])
        assert nl.get_tersoff()["lds"] == lds

    calls = {"sw forces": (None, lambda: nl.sw_forces(qd, out=f)), "sw virial": (None, lambda: nl.sw_virial(qd, out=out))}
    nl.sw_forces(qd, out=f), nl.sw_virial(qd, out=out)
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(out).all()), "a centre with more than 64 partners in range"
    if not YARDSTICK:
        calls.update({
            "tersoff forces, LDS": (True, lambda: nl.tersoff_forces(qd, out=f)),
            "tersoff forces, global": (False, lambda: nl.tersoff_forces(qd, out=f)),
            "tersoff virial, LDS": (True, lambda: nl.tersoff_virial(qd, out=out)),
            "tersoff virial, global": (False, lambda: nl.tersoff_virial(qd, out=out)),
        })
        tables(True)
        nl.tersoff_forces(qd, out=f), nl.tersoff_virial(qd, out=out)
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(out).all()), "a centre with more than 64 partners in range"
        kp, lst, _ = nl.full_csr()
        kp, lst = kp.long(), lst.long()
        rows = torch.repeat_interleave(torch.arange(len(q), device="cuda"), kp[1:] - kp[:-1])
        d = qd[rows, :3] - qd[lst, :3]
        L = torch.tensor(w["box"], dtype=torch.float32, device="cuda")
        d = d - torch.round(d / L) * L
        m = torch.bincount(rows[(d * d).sum(dim=1) < w["r3"] ** 2], minlength=len(q)).double()
        print(f"{name}: n {len(q)}, entries {len(rows)}, partners within {w['r3']:g} mean {float(m.mean()):.2f} max {int(m.max())}, "
              f"ordered pairs of partners {float((m * (m - 1)).sum()):.4e}, E {float(out[6]):.6e}", flush=True)
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
        ref = np.median(ms["sw forces" if "forces" in k else "sw virial"])
        print(f"{name}, {k:24s}: median {np.median(v):.3f} ms (batches {v.min():.3f} .. {v.max():.3f}), {np.median(v) / ref:.3f} x sw", flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, make in (("cfg2", cfg2), ("silicon", silicon)):
        if not only or name in only:
            run(name, make())


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""An MD loop around the list: velocity Verlet for a Lennard-Jones droplet with
  * a Verlet list built with cut-off rc + skin, reused until some particle has moved more than skin / 2
    (max displacement since the last build), then rebuilt;
  * every SORT_FREQ rebuilds (the reference declares SORT_FREQ = 50 and never uses it, neighlist_gpu.hpp:72) the
    particle arrays are permuted into the build's cell order (nl_resort), which speeds up both the next builds
    and the force gathers (profiles/r01_force_consumer_timing.txt);
  * forces from nl_lj_forces on the full list (one gather per row, no atomics).
The list has no minimum image by default (neither has the reference): the droplet sits in the middle of an open box.
--periodic xyz fills the whole box with the crystal and takes the minimum image on every axis; --periodic xy is a film
that fills x and y (minimum image there, nl_set_periodic_axes) and is finite in z, in the middle of an open z range.
On the periodic axes the positions are wrapped back into [0, L) after every drift; the displacement since the last
build is taken at the minimum image there (the host trigger as rule (c) of nl_update_list does).

The rebuild trigger (--trigger):
  host    the displacement since the last build is reduced on the device and compared on the host: one host sync per
          step, plus the one nl_lj_forces makes;
  device  nl_update_list decides on the device and rebuilds only when needed, nl_lj_forces_enqueue does not wait: a step
          is enqueued without a host sync; --graph captures one whole step (integrate, update, forces) into a
          torch.cuda.graph and replays it.  The re-sort reads update_stats() every SORT_CHECK steps.

--pressure prints P = N kT / V + tr W / (3 V) at the end, W from nl_lj_virial on the loop's list (V: the whole box).

--dpd GAMMA KT adds the DPD pair thermostat (nl_set_dpd over a pair table of zeros, weight 1 - r / rc): f = lj_forces +
dpd_forces, the friction taken at the velocities of the force evaluation, sigma = sqrt(2 GAMMA KT).  The step word of the
noise lives on the device and is advanced inside the step, so a captured step draws fresh noise at every replay.  The run
then also prints the kinetic temperature, averaged over its second half, against KT, and the drift of the total momentum.

usage: tools/md_loop.py [--cells 12] [--steps 400] [--dtype f64] [--trigger host|device] [--graph]
                        [--periodic none|xyz|xy] [--pressure] [--dpd GAMMA KT]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_neighbor_list_amd import NeighListGPU, dpd  # noqa: E402

SORT_FREQ = 50
SORT_CHECK = 50  # device trigger: steps between two looks at the build count (a host sync)
DPD_R_MIN, DPD_KNOTS, DPD_SEED = 0.5, 512, 2024  # the weight table's grid (the LJ core keeps every pair beyond 0.5) and the seed


def fcc_droplet(cells, a, box, dtype, seed=1):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((g + base).reshape(-1, 3) * a).astype(np.float64)
    pos += 0.5 * (box - cells * a)
    rng = np.random.default_rng(seed)
    vel = rng.normal(0.0, 0.3, size=pos.shape)
    vel -= vel.mean(axis=0)
    q = np.zeros((len(pos), 4), dtype=dtype)
    q[:, :3] = pos
    return q, vel.astype(dtype)


def fcc_slab(cells, a, box, dtype, seed=1):
    """An FCC crystal of cells[0] x cells[1] x cells[2] unit cells (edge a) centred in a box of edges box[0..2]: with
    cells[d] * a == box[d] it fills that axis (periodic), with fewer cells it leaves a gap (an open axis)."""
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((g + base).reshape(-1, 3) * a + 0.25 * a).astype(np.float64)
    pos += 0.5 * (np.array(box, dtype=np.float64) - np.array(cells) * a)
    rng = np.random.default_rng(seed)
    vel = rng.normal(0.0, 0.3, size=pos.shape)
    vel -= vel.mean(axis=0)
    q = np.zeros((len(pos), 4), dtype=dtype)
    q[:, :3] = pos
    return q, vel.astype(dtype)


class Simulation:
    def __init__(self, q, v, box, rc=2.5, skin=0.4, dt=0.004, device="cuda", trigger="host", graph=False, periodic="", thermostat=None):
        if trigger not in ("host", "device") or (graph and trigger != "device"):
            raise ValueError("trigger is 'host' or 'device'; graph needs the device trigger")
        self.trigger, self.use_graph, self.graph, self.steps = trigger, graph, None, 0
        self.tdt = torch.float32 if q.dtype == np.float32 else torch.float64
        self.q = torch.from_numpy(q).to(device)
        self.v = torch.from_numpy(v).to(device)
        self.ids = torch.arange(len(q), device=device)  # original identity of every slot (changes when re-sorted)
        self.rc, self.skin, self.dt, self.box = rc, skin, dt, box
        # periodic: the axes of the minimum image ("" = the open box); box: one edge, or three
        self.edges = tuple(box) if np.ndim(box) else (box, box, box)
        self.axes = [d for d in range(3) if "xyz"[d] in periodic]
        self.nl = NeighListGPU(rc + skin, *self.edges, dtype=self.tdt, full_list=True)
        if self.axes:
            self.nl.set_periodic(axes=periodic)
        self.nl.Initialize(len(q))
        self.builds = self.sorts = 0
        self.q_built = None
        # thermostat: (gamma, kT) of the DPD pair term, over a pair table of zeros; ke_sum: sum of v^2 over the steps since
        # it was last zeroed, kept on the device
        self.thermostat = thermostat
        self.ke_sum = torch.zeros((), dtype=torch.float64, device=device)
        if thermostat is not None:
            gamma, kT = thermostat
            zeros = np.zeros(DPD_KNOTS)
            self.nl.set_pair_table(zeros, zeros, DPD_R_MIN, rc)
            self.nl.set_dpd(dpd.weight(DPD_R_MIN, rc, DPD_KNOTS), gamma, dpd.sigma_for(gamma, kT), DPD_R_MIN, rc, dt, DPD_SEED)
            self.step_word = torch.zeros(1, dtype=torch.int64, device=device)
            self.fd = torch.empty((len(q), 4), dtype=self.tdt, device=device)
        if trigger == "device":
            self.nl.set_skin(skin)
            self.nl.update(self.q, sync=True)
            self.sorted_at = 0  # build count at the last re-sort
            self.f = torch.empty((len(q), 4), dtype=self.tdt, device=device)
            self.forces(wait=False)
            return
        self.rebuild()
        self.f = torch.empty((len(q), 4), dtype=self.tdt, device=device)
        self.forces(wait=True)

    def forces(self, wait):
        """f = lj_forces, plus dpd_forces at the current velocities and step word, which is then advanced on the device."""
        self.nl.lj_forces(self.q, 1.0, 1.0, rc_force=self.rc, wait=wait, out=self.f)
        if self.thermostat is not None:
            self.nl.dpd_forces(self.q, self.v, self.step_word, wait=wait, out=self.fd)
            self.f += self.fd
            self.step_word += 1

    def rebuild(self):
        if self.builds and self.builds % SORT_FREQ == 0:
            # re-sort: the previous build's cell order becomes the storage order (nl_resort, in place)
            self.nl.resort(self.q, self.v, self.ids)
            self.sorts += 1
        self.nl.MakeNeighList(self.q, len(self.q))
        self.q_built = self.q.clone()
        self.builds += 1

    def step(self):
        if self.trigger == "device":
            return self.step_device()
        dt = self.dt
        self.v += 0.5 * dt * self.f[:, :3]
        self.q[:, :3] += dt * self.v
        self.wrap()
        d = self.q[:, :3] - self.q_built[:, :3]
        for a in self.axes:  # (minimum image on the periodic axes)
            d[:, a] -= self.edges[a] * torch.round(d[:, a] / self.edges[a])
        moved = d.square().sum(dim=1).max()
        if float(moved) > (0.5 * self.skin) ** 2:  # (one host sync per step: the rebuild decision)
            self.rebuild()
        self.forces(wait=True)
        self.v += 0.5 * dt * self.f[:, :3]
        self.ke_sum += self.v.square().sum()

    def wrap(self):
        """Periodic axes: positions back into [0, L) (the list takes every pair at its minimum image)."""
        for a in self.axes:
            self.q[:, a] -= self.edges[a] * torch.floor(self.q[:, a] / self.edges[a])

    def _device_step(self):
        dt = self.dt
        self.v += 0.5 * dt * self.f[:, :3]
        self.q[:, :3] += dt * self.v
        self.wrap()
        self.nl.update(self.q)  # (the rebuild decision on the device, no host sync)
        self.forces(wait=False)
        self.v += 0.5 * dt * self.f[:, :3]
        self.ke_sum += self.v.square().sum()

    def step_device(self):
        if self.steps and self.steps % SORT_CHECK == 0:
            builds = self.nl.update_stats()[1]
            if builds - self.sorted_at >= SORT_FREQ:
                # re-sort into the last build's cell order (f too: the next step starts from it); the update after a
                # re-sort builds, here outside any graph
                self.nl.resort(self.q, self.v, self.ids, self.f)
                self.nl.update(self.q, sync=True)
                self.sorted_at = builds + 1
                self.sorts += 1
        if self.use_graph and self.graph is None and self.steps >= 1:  # (the first step runs eagerly: warm-up)
            self.nl.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._device_step()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._device_step()
        self.steps += 1

    def build_count(self):
        return self.nl.update_stats()[1] if self.trigger == "device" else self.builds

    def temperature_since(self, steps):
        """The mean kinetic temperature sum v^2 / (3 N - 3) over the last `steps` steps; zeroes the sum (one host sync)."""
        t = float(self.ke_sum) / (steps * (3 * len(self.q) - 3))
        self.ke_sum.zero_()
        return t

    def momentum(self):
        return self.v.to(torch.float64).sum(dim=0).cpu().numpy()

    def energy(self):
        return float(self.f[:, 3].sum() + 0.5 * self.v.square().sum())

    def pressure(self):
        """(P, U) from nl_lj_virial on the current list: P = N kT / V + tr W / (3 V) with N kT = sum v^2 / 3."""
        self.nl.synchronize()  # (the device trigger's last update may sit on a captured step's stream)
        w = self.nl.lj_virial(self.q, 1.0, 1.0, rc_force=self.rc)
        volume = float(np.prod(self.edges))
        return float(self.v.square().sum() / 3.0 + w[:3].sum() / 3.0) / volume, float(w[6])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=12)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"])
    ap.add_argument("--trigger", default="host", choices=["host", "device"])
    ap.add_argument("--graph", action="store_true", help="device trigger: replay one captured step")
    ap.add_argument("--periodic", default="none", choices=["none", "xyz", "xy"],
                    help="minimum image: none (a droplet in an open box), xyz (a crystal filling the box), xy (a film)")
    ap.add_argument("--pressure", action="store_true", help="print the pressure and the potential energy from nl_lj_virial")
    ap.add_argument("--dpd", type=float, nargs=2, metavar=("GAMMA", "KT"), help="the DPD pair thermostat: friction and temperature")
    args = ap.parse_args()
    a, box = 1.56, 4.0 * args.cells
    dt_np = np.float32 if args.dtype == "f32" else np.float64
    if args.periodic == "none":
        q, v = fcc_droplet(args.cells, a, box, dt_np)
        sim = Simulation(q, v, box, trigger=args.trigger, graph=args.graph, thermostat=args.dpd)
    else:
        c = args.cells
        cells = (c, c, c) if args.periodic == "xyz" else (c, c, max(c // 2, 2))
        edges = (c * a, c * a, c * a if args.periodic == "xyz" else box)
        q, v = fcc_slab(cells, a, edges, dt_np)
        sim = Simulation(q, v, edges, trigger=args.trigger, graph=args.graph, periodic=args.periodic, thermostat=args.dpd)
    e0, p0 = sim.energy(), sim.momentum()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        if args.dpd and k == args.steps // 2:
            sim.temperature_since(max(k, 1))  # (the second half starts here)
        sim.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e1 = sim.energy()
    print(f"N={len(q)} periodic={args.periodic} trigger={args.trigger}{'+graph' if args.graph else ''} steps={args.steps} builds={sim.build_count()} "
          f"re-sorts={sim.sorts} E0={e0:.6f} E1={e1:.6f} "
          f"drift={(e1 - e0) / abs(e0):.2e} {1e3 * dt / args.steps:.3f} ms/step")
    if args.dpd:
        t2 = sim.temperature_since(args.steps - args.steps // 2)
        print(f"DPD gamma={args.dpd[0]:g} kT={args.dpd[1]:g}: kinetic temperature over the second half {t2:.4f} ({t2 / args.dpd[1]:.4f} kT); "
              f"total momentum {np.abs(p0).max():.3e} -> {np.abs(sim.momentum()).max():.3e} (largest component)")
    if args.pressure:
        p, u = sim.pressure()
        print(f"P={p:.6f} U={u:.6f} (nl_lj_virial)")


if __name__ == "__main__":
    main()

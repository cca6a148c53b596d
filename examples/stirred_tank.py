#!/usr/bin/env python3
"""
A stirred tank: a closed 3-D box of fluid and a horizontal rod -- `cylinder(..., axis='x')`, phi/geom/_cylinder.py of PhiFlow -- that turns about the vertical
axis through its centre. The rod is an `Obstacle` with an angular velocity about z and is re-posed every step with `obstacle.rotated(Rz(omega dt))`, as
examples/grids/Rotating_Bar.ipynb does with its box; the step is semi-Lagrangian self-advection + make_incompressible(v, obstacle, Solve(x0=p)).
The analytic cylinder is rasterised inside the obstacle kernels each step: nothing is re-sampled on the host. Every 10 steps the script prints the kinetic
energy and the largest |divergence| on fluid cells.
    python examples/stirred_tank.py [--size 48] [--steps 100]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import Box, Obstacle, Solve, StaggeredGrid, advect, cylinder, divergence, fluid   # noqa: E402

DOMAIN = Box(x=100, y=100, z=100)
OMEGA = 0.05                 # rad per unit time, about z
ROD = dict(x=50, y=50, z=50, radius=6, depth=60)


def rz(angle: float) -> np.ndarray:
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def time_step(size: int) -> float:
    """ CFL 0.5 on the speed of the rod's tips """
    return 0.5 * (DOMAIN.size[0] / size) / (OMEGA * 0.5 * ROD['depth'])


def make_obstacle() -> Obstacle:
    return Obstacle(cylinder(axis='x', **ROD), angular_velocity=(0, 0, OMEGA))


def fluid_cells(v, obstacle) -> np.ndarray:
    pts = [l + (np.arange(n) + 0.5) * (u - l) / n for l, u, n in zip(v.bounds.lower, v.bounds.upper, v.resolution.values())]
    return ~obstacle.geometry.lies_inside(np.meshgrid(*pts, indexing='ij'))


def run(size: int = 48, steps: int = 100, backend=None, log=print):
    obstacle = make_obstacle()
    v = StaggeredGrid(0, 0, DOMAIN, x=size, y=size, z=size, backend=backend)
    p = None
    dt = time_step(size)
    cell = float(np.prod([s / size for s in DOMAIN.size]))
    worst = 0.0
    for k in range(1, steps + 1):
        obstacle = obstacle.rotated(rz(OMEGA * dt))
        v = advect.semi_lagrangian(v, v, dt)
        v, p = fluid.make_incompressible(v, obstacle, Solve('CG', 1e-5, 1e-5, x0=p))
        if k % 10 == 0 or k == steps:
            d = float(np.abs(divergence(v).numpy()[fluid_cells(v, obstacle)]).max())
            worst = max(worst, d)
            energy = 0.5 * cell * sum(float((a.astype(np.float64) ** 2).sum()) for a in v.numpy())
            log(f"step {k:4d}: kinetic energy {energy:.5e}, max |div| on fluid cells {d:.3e}")
            assert math.isfinite(d) and math.isfinite(energy), "non-finite values"
    return v, p, obstacle, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=48, help="cells per axis")
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    t0 = time.perf_counter()
    v, p, obstacle, worst = run(args.size, args.steps)
    print(f"{args.steps} steps at {args.size}^3 in {time.perf_counter() - t0:.2f} s, worst max |div| {worst:.3e}")


if __name__ == "__main__":
    main()

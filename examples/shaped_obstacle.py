#!/usr/bin/env python3
"""
Wake flow around a NACA 0012 section at an angle of attack -- a shape no Box / Sphere composition describes, given to the solver as a grid of
signed distances (`SDFGrid`, phi/geom/_sdf_grid.py of PhiFlow). The set-up follows examples/grids/Wake_Flow.ipynb in 2-D: constant inflow at x-,
open x+, periodic y; the step is semi-Lagrangian self-advection + make_incompressible(v, obstacle, Solve(x0=p)), `jit_compile`'d.
The SDF is built once, in NumPy: at every cell centre of its grid the distance to the section's outline (a closed polyline), negative inside
(point-in-polygon by ray crossing). Every 10 steps the script prints the largest |divergence| on fluid cells.
    python examples/shaped_obstacle.py [--size 128] [--steps 100] [--angle 12]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import PERIODIC, ZERO_GRADIENT, Box, Obstacle, SDFGrid, Solve, StaggeredGrid, advect, divergence, fluid, jit_compile, vec   # noqa: E402

DOMAIN = Box(x=200, y=100)
INFLOW = 2.0


def naca0012_outline(chord: float, angle_deg: float, le_x: float, le_y: float, n: int = 120) -> np.ndarray:
    """ closed polyline [2 n, 2] of a NACA 0012 section (half thickness 0.6 (0.2969 sqrt(x) - 0.1260 x - 0.3516 x^2 + 0.2843 x^3 - 0.1036 x^4), closed
    trailing edge), pitched nose-up by angle_deg about its leading edge at (le_x, le_y) """
    x = 0.5 * (1 - np.cos(np.linspace(0, np.pi, n)))            # cosine spacing: points crowd at both edges
    t = 0.6 * (0.2969 * np.sqrt(x) - 0.1260 * x - 0.3516 * x ** 2 + 0.2843 * x ** 3 - 0.1036 * x ** 4)
    pts = np.concatenate([np.stack([x, t], 1), np.stack([x[::-1], -t[::-1]], 1)]) * chord
    a = -math.radians(angle_deg)                                 # inflow along +x: nose-up = clockwise in (x, y)
    rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return pts @ rot.T + np.array([le_x, le_y])


def polygon_sdf(outline: np.ndarray, bounds: Box, res) -> np.ndarray:
    """ signed distance to the closed polyline at the cell centres of `bounds` (res cells per axis): distance to the nearest segment, sign by the crossing
    number of a ray along +x """
    xs = [l + (np.arange(n) + 0.5) * (u - l) / n for l, u, n in zip(bounds.lower, bounds.upper, res)]
    px, py = np.meshgrid(xs[0], xs[1], indexing='ij')
    a, b = outline, np.roll(outline, -1, axis=0)
    dist2 = np.full(px.shape, np.inf)
    inside = np.zeros(px.shape, bool)
    for (ax, ay), (bx, by) in zip(a, b):
        ex, ey = bx - ax, by - ay
        t = np.clip(((px - ax) * ex + (py - ay) * ey) / max(ex * ex + ey * ey, 1e-300), 0.0, 1.0)
        dist2 = np.minimum(dist2, (px - ax - t * ex) ** 2 + (py - ay - t * ey) ** 2)
        if ay != by:
            crosses = ((ay > py) != (by > py)) & (px < ax + (py - ay) / (by - ay) * ex)
            inside ^= crosses
    return np.where(inside, -1.0, 1.0) * np.sqrt(dist2)


def make_obstacle(size: int, angle_deg: float = 12.0) -> Obstacle:
    """ the section (chord 50) inside SDF bounds that leave a margin of a few cells; two SDF cells per simulation cell """
    outline = naca0012_outline(50.0, angle_deg, 40.0, 54.0)
    lo, hi = outline.min(0) - 6.0, outline.max(0) + 6.0
    bounds = Box(x=(float(lo[0]), float(hi[0])), y=(float(lo[1]), float(hi[1])))
    h = DOMAIN.size[0] / (2 * size) / 2
    res = [max(8, int(math.ceil(s / h))) for s in bounds.size]
    sdf = polygon_sdf(outline, bounds, res).astype(np.float32)
    return Obstacle(SDFGrid(sdf, bounds))


def initial_velocity(size: int, backend=None):
    boundary = {'x-': vec(x=INFLOW, y=0), 'x+': ZERO_GRADIENT, 'y': PERIODIC}
    return StaggeredGrid((INFLOW, 0), boundary, x=2 * size, y=size, bounds=DOMAIN, backend=backend)


def max_fluid_divergence(v, obstacle) -> float:
    """ largest |div v| over the cells whose centre lies outside the obstacle """
    div = divergence(v).numpy()
    pts = [l + (np.arange(n) + 0.5) * (u - l) / n for l, u, n in zip(v.bounds.lower, v.bounds.upper, v.resolution.values())]
    fluid_cells = ~obstacle.geometry.lies_inside(np.meshgrid(*pts, indexing='ij'))
    return float(np.abs(div[fluid_cells]).max())


def run(size: int = 128, steps: int = 100, angle_deg: float = 12.0, backend=None, log=print):
    obstacle = make_obstacle(size, angle_deg)
    v = initial_velocity(size, backend)
    dt = 0.5 * (DOMAIN.size[0] / (2 * size)) / INFLOW            # CFL 0.5 on the inflow speed
    # multigrid-preconditioned CG: the iteration count does not grow with the grid (plain CG needs > 1000 iterations for the first projection at 512 x 256)
    v, p = fluid.make_incompressible(v, obstacle, Solve('CG', 1e-5, 1e-5, preconditioner='multigrid'))

    @jit_compile
    def step(v, p):      # captured: the host is not told how the solve went, so the solve gets a launch budget that fits a warm start
        v = advect.semi_lagrangian(v, v, dt)
        return fluid.make_incompressible(v, obstacle, Solve('CG', 1e-5, 1e-5, x0=p, max_iterations=15, preconditioner='multigrid'))

    worst = 0.0
    for k in range(1, steps + 1):
        v, p = step(v, p)
        if k % 10 == 0 or k == steps:
            d = max_fluid_divergence(v, obstacle)
            worst = max(worst, d)
            log(f"step {k:4d}: max |div| on fluid cells {d:.3e}, max |v_y| {float(np.abs(v.numpy()[1]).max()):.4f}")
            assert math.isfinite(d), "non-finite values"
    return v, p, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="cells along y; the grid is 2 size x size")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--angle", type=float, default=12.0, help="angle of attack in degrees")
    args = ap.parse_args()
    t0 = time.perf_counter()
    v, p, worst = run(args.size, args.steps, args.angle)
    print(f"{args.steps} steps at {2 * args.size} x {args.size} in {time.perf_counter() - t0:.2f} s, worst max |div| {worst:.3e}")


if __name__ == "__main__":
    main()

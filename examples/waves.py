#!/usr/bin/env python3
"""
Wave equation with a moving source (examples/grids/Waves.ipynb of PhiFlow, with the import line changed): a height field on a ZERO_GRADIENT
grid over Box(x=12.8, y=12.8),
    h_next = 2 h - h_prev + dt^2 (k_speed * laplace(h) - k_damp * (h - h_prev)),
with `field.where(sphere, mag * sin(t), h)` pressing a sphere of radius 1 into both time levels before every step. The sphere circles the
centre of the domain: the notebook's `math.rotate_vector(vec(x=0, y=-12.8/3), time)` is two lines of trigonometry here. The sphere is
rasterised on the host from the Python number `time`, so the step runs eagerly (a capture would bake the mask in).
Every 10 steps the script prints max |h| and fails if anything is non-finite.
    python examples/waves.py [--size 128] [--steps 100]
"""
import argparse
import math
import os
import sys
import time as _time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import ZERO_GRADIENT, Box, CenteredGrid, Sphere, field   # noqa: E402

DT = 1 / 60. / 16


def wave_displace(sphere, *fields, mag=.5, t=-math.pi * 0.5):
    return [field.where(sphere, mag * math.sin(t), f) for f in fields]


def step(h_c, h_p, time, dt=DT, k_speed=1.0, k_damp=0.0):
    ox, oy = 0.0, -12.8 / 3         # rotate_vector((0, -12.8 / 3), time)
    rx, ry = math.cos(time) * ox - math.sin(time) * oy, math.sin(time) * ox + math.cos(time) * oy
    cx, cy = [0.5 * (lo + up) for lo, up in zip(h_c.bounds.lower, h_c.bounds.upper)]
    sphere = Sphere(x=cx + rx, y=cy + ry, radius=1.)
    h_c, h_p = wave_displace(sphere, h_c, h_p)
    h_n = 2.0 * h_c - h_p + dt * dt * (k_speed * h_c.laplace() - k_damp * (h_c - h_p))  # wave_solve
    return h_n, h_c, time + dt


def initial_height(size: int = 128, backend=None):
    return CenteredGrid(0, ZERO_GRADIENT, Box(x=12.8, y=12.8), x=size, y=size, backend=backend)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    h_c = h_p = initial_height(args.size)
    t = 0.0
    t0 = _time.perf_counter()
    for k in range(1, args.steps + 1):
        h_c, h_p, t = step(h_c, h_p, t)
        if k % 10 == 0 or k == args.steps:
            m = float(h_c.values.abs().max())
            print(f"step {k:4d}: max |h| {m:.6f}")
            assert math.isfinite(m), "non-finite values"
    print(f"{args.steps} steps at {args.size}^2 in {_time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()

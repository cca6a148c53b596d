#!/usr/bin/env python3
"""
Burgers' equation in 2-D (examples/grids/Burgers.ipynb of PhiFlow, 2-D case, with the import line changed): a centred velocity on a periodic
64 x 64 grid spanning Box(x=40, y=20), initialised with smooth noise, is diffused implicitly and then advected by itself each step. The
jit_compile'd step runs under `iterate` for 100 steps. Every 10 steps the script prints the kinetic energy and max |v_c| per component:
on a periodic grid both operations obey a maximum principle (linear semi-Lagrangian interpolation is a convex combination, (I - k dt L)^-1 is
non-negative with unit row sums), so max |v_c| must not grow and the energy decays.
    python examples/burgers.py [--size 64] [--steps 100]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import Box, CenteredGrid, Noise, PERIODIC, advect, diffuse, iterate, jit_compile   # noqa: E402

DT = 0.5       # `def step(v, dt=.5)` in the notebook


def initial_velocity(size: int = 64, backend=None):
    """ v0 = CenteredGrid(Noise(vector='x,y'), PERIODIC, x=size, y=size, bounds=Box(x=40, y=20)) """
    return CenteredGrid(Noise(vector='x,y'), PERIODIC, x=size, y=size, bounds=Box(x=40, y=20), backend=backend)


def step(v, dt: float = DT):
    v = diffuse.implicit(v, 0.1, dt)
    v = advect.semi_lagrangian(v, v, dt)
    return v


def kinetic_energy(v) -> float:
    """ 0.5 * sum |v|^2 * cell volume """
    return 0.5 * float((v.values.double() ** 2).sum()) * float(np.prod(v.dx))


def max_abs(v):
    """ max |v_c| per component """
    return [float(v.values[:, c].abs().max()) for c in range(v.spatial_rank)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    v = initial_velocity(args.size)
    jit_step = jit_compile(step)
    e0, m0 = kinetic_energy(v), max_abs(v)
    print(f"step    0: energy {e0:.6f}, max |v_x| {m0[0]:.5f}, max |v_y| {m0[1]:.5f}")
    t0 = time.perf_counter()
    done = 0
    while done < args.steps:
        n = min(10, args.steps - done)
        v = iterate(jit_step, n, v)
        done += n
        e, m = kinetic_energy(v), max_abs(v)
        print(f"step {done:4d}: energy {e:.6f}, max |v_x| {m[0]:.5f}, max |v_y| {m[1]:.5f}")
        assert all(a <= b * (1 + 1e-4) for a, b in zip(m, m0)), "maximum principle violated"
    assert kinetic_energy(v) < e0
    print(f"{args.steps} steps in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()

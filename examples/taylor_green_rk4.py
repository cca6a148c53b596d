#!/usr/bin/env python3
"""
Decaying 2-D Taylor-Green vortex with viscosity, twice: the method-of-lines step -- `fluid.incompressible_rk4` over
`advect.differential` + `diffuse.differential`, the Runge-Kutta step that carries the pressure through its stages -- and the operator-split step
`advect.semi_lagrangian -> diffuse.explicit -> make_incompressible`. The kinetic energy of the exact solution decays like exp(-4 nu t): the script prints both
measured ratios next to it. The split step loses a good part of the energy to the interpolation of the advection scheme; the error of the
Runge-Kutta step is the second-order error of the central differences (+0.4 % at 16^2, +0.1 % at 32^2 for nu = 0.1, T = 0.8). Needs an MI355X.
    python examples/taylor_green_rk4.py [--size 32] [--steps 8] [--nu 0.1]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import *   # noqa: E402,F401,F403


def momentum(v, nu):
    """ every term of the momentum equation but the pressure's """
    return advect.differential(v, v) + diffuse.differential(v, nu)


def rk4_step(v, p, dt, nu, solve):
    return fluid.incompressible_rk4(momentum, v, p, dt, pressure_order=2, pressure_solve=solve, nu=nu)


def split_step(v, p, dt, nu, solve):
    v = advect.semi_lagrangian(v, v, dt)
    v = diffuse.explicit(v, nu, dt)
    return fluid.make_incompressible(v, (), solve)


def initial_fields(n, backend=None):
    L = 2 * math.pi
    box = Box(x=L, y=L)
    v = StaggeredGrid(lambda x, y: (np.sin(x) * np.cos(y), -np.cos(x) * np.sin(y)), PERIODIC, box, x=n, y=n, backend=backend)
    return v, CenteredGrid(0, PERIODIC, box, x=n, y=n, backend=backend)


def energy(v):
    return sum(float((c.astype('float64') ** 2).sum()) for c in v.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--dt", type=float, default=0.1)
    args = ap.parse_args()
    with precision(64):
        solve = Solve('CG', 1e-10, 1e-10)
        exact = math.exp(-4 * args.nu * args.steps * args.dt)
        print(f"{args.steps} steps of dt = {args.dt} at {args.size}^2, nu = {args.nu}: exact E(T) / E(0) = {exact:.6f}")
        for name, step in (("incompressible_rk4", rk4_step), ("split step", split_step)):
            v, p = initial_fields(args.size)
            e0 = energy(v)
            for _ in range(args.steps):
                v, p = step(v, p, args.dt, args.nu, solve)
            ratio = energy(v) / e0
            print(f"  {name:20s} E(T) / E(0) = {ratio:.6f}   error {ratio / exact - 1:+.3%}")


if __name__ == "__main__":
    main()

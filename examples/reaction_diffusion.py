#!/usr/bin/env python3
"""
Gray-Scott reaction-diffusion (examples/grids/Reaction_Diffusion.ipynb of PhiFlow, with the import line changed): two species u, v on a
periodic grid with dx = 1,
    uvv = u * v**2
    u' = du * laplace(u) - uvv + f * (1 - u)
    v' = dv * laplace(v) + uvv - (f + k) * v
integrated with explicit Euler steps of dt = 0.5. The step is jit_compile'd and runs under `iterate`; `field.laplace` is the only stencil.
Parameter sets of the notebook: maze, coral, dots. Every 10 steps the script prints max |u| and max |v| and fails if anything is non-finite.
    python examples/reaction_diffusion.py [--size 100] [--steps 100] [--pattern maze]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import PERIODIC, CenteredGrid, field, iterate, jit_compile   # noqa: E402

DT = 0.5
PATTERNS = {
    'maze': {'du': 0.19, 'dv': 0.05, 'f': 0.06, 'k': 0.062},
    'coral': {'du': 0.16, 'dv': 0.08, 'f': 0.06, 'k': 0.062},
    'dots': {'du': 0.19, 'dv': 0.03, 'f': 0.04, 'k': 0.061},
}


def reaction_diffusion(u, v, du, dv, f, k, dt):
    uvv = u * v ** 2
    su = du * field.laplace(u) - uvv + f * (1 - u)
    sv = dv * field.laplace(v) + uvv - (f + k) * v
    return u + dt * su, v + dt * sv


def initial_field(size: int, backend=None):
    """ the notebook's second initialisation: a Gaussian bump of width 3 in the middle of the grid (used for both species) """
    c = 0.5 * size
    return CenteredGrid(lambda x, y: np.exp(-0.5 * ((x - c) ** 2 + (y - c) ** 2) / 3 ** 2), PERIODIC, x=size, y=size, backend=backend)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--pattern", choices=sorted(PATTERNS), default='maze')
    args = ap.parse_args()
    prm = PATTERNS[args.pattern]
    u = initial_field(args.size)
    v = initial_field(args.size)
    step = jit_compile(lambda u, v: reaction_diffusion(u, v, dt=DT, **prm))
    t0 = time.perf_counter()
    done = 0
    while done < args.steps:
        n = min(10, args.steps - done)
        u, v = iterate(step, n, u, v)
        done += n
        mu, mv = float(u.values.abs().max()), float(v.values.abs().max())
        print(f"step {done:4d}: max |u| {mu:.6f}, max |v| {mv:.6f}")
        assert math.isfinite(mu) and math.isfinite(mv), "non-finite values"
    print(f"{args.steps} steps of '{args.pattern}' at {args.size}^2 in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()

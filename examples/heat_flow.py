#!/usr/bin/env python3
"""
Heat flow through a conducting structure: implicit diffusion with a spatially varying conductivity. Two crossing bars conduct well
(conductivity 1.01), the rest of the box poorly (0.01); the left wall is held at temperature 1, the right wall is insulated (zero
gradient) and the box is periodic along y. Every step solves  (I - dt div(k grad)) T_new = T  with CG on the flux-form operator of
csrc/diffuse_coef.hpp; the step is jit_compile'd (captured once, replayed after). Prints the mean temperature inside and outside the bars.
    python examples/heat_flow.py [--steps 100] [--dt 1.0] [--nx 100] [--ny 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiflow_amd.flow import Box, CenteredGrid, PERIODIC, ZERO_GRADIENT, diffuse, jit_compile, union   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=1.0)
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--ny", type=int, default=50)
    args = ap.parse_args()
    domain = Box(x=10, y=5)
    structure = union(Box(x=(0, 10), y=(2, 3)), Box(x=(4.5, 5.5), y=(1, 4)))
    conductivity = CenteredGrid(structure, ZERO_GRADIENT, domain, x=args.nx, y=args.ny) + 0.01
    temperature = CenteredGrid(0, {'x-': 1, 'x+': ZERO_GRADIENT, 'y': PERIODIC}, domain, x=args.nx, y=args.ny)

    @jit_compile
    def step(t, dt):
        return diffuse.implicit(t, conductivity, dt)

    inside = conductivity.numpy() > 0.5
    t0 = time.perf_counter()
    for i in range(args.steps):
        temperature = step(temperature, args.dt)
        if (i + 1) % max(1, args.steps // 5) == 0:
            vals = temperature.numpy()
            print(f"step {i + 1:4d}: mean T in the bars {vals[inside].mean():.4f}, elsewhere {vals[~inside].mean():.4f}, "
                  f"range [{vals.min():.4f}, {vals.max():.4f}]")
    vals = temperature.numpy()
    assert np.isfinite(vals).all() and vals.min() >= -1e-4 and vals.max() <= 1 + 1e-4
    print(f"{args.steps} steps in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()

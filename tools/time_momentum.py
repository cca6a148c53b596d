#!/usr/bin/env python3
"""
The finite-difference advection term on the MI355X (csrc/momentum.hpp), in one process, every group ALTERNATING and the best of a few repetitions
(as tools/time_diffops.py):
  advect.differential(v, v)               against advect.semi_lagrangian(v, v, dt) and field.laplace(v) on the same staggered field, at
                                          256^3 fp32 periodic, 384^3 fp64 closed and 2048^2 x 8 fp32 periodic
  the centred form at 256^3 fp32          against the centred gradient of one scalar (cgrad_kernel)
  one RK4 step                            against one split step (semi_lagrangian + diffuse.explicit + make_incompressible) at 256^3 fp32, Solve('CG', 1e-5), warm; the split step's solve starts from x0 = p,
                                          the stage solves of the RK4 step (pressure increments) from 0
Prints one JSON line per measurement: ms per call and the fraction of 8 TB/s BY NEED -- 2 D words per cell for the advection forms (D components in,
D out), 2 D for the staggered laplace, 1 + D for the gradient. Repeated calls on arrays of 64 MB are Infinity-Cache-warm: only the ratios measured in
this one process count. Fails without a GPU.
    python tools/time_momentum.py [--reps 100] [--rounds 5] [--skip-steps]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phiflow_amd import _capi as C   # noqa: E402

PEAK = 8e12


def alternate(fns, reps, rounds):
    """ best time per call of every function, the functions taking turns `rounds` times """
    for fn in fns.values():
        for _ in range(3):
            fn()
    best = {k: float('inf') for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            best[k] = min(best[k], (time.perf_counter() - t0) / reps)
    return best


def report(what, config, cells, esize, t, words, ref=None):
    rate = words * esize * cells / t / PEAK
    line = {"what": what, "config": config, "ms": t * 1e3, "words_per_cell": words, "of_8TBs_by_need": rate}
    for name, t_ref in (ref or {}).items():
        line[f"time_over_{name}"] = t / t_ref
    print(json.dumps(line), flush=True)


def staggered_group(ctx, dev, g, config, res, batch, dtype, code, reps, rounds):
    D = len(res)
    tdt, cdt, esize = (torch.float32, C.PHIHIP_F32, 4) if dtype == "f32" else (torch.float64, C.PHIHIP_F64, 8)
    bc = ((code, code),) * D
    grid = C.make_grid(D, cdt, batch, res, (0,) * D, tuple(float(n) for n in res), bc)
    shapes = []
    for d in range(D):
        s = list(res)
        s[d] += {C.BC_PERIODIC: 0, C.BC_CLOSED: -1, C.BC_OPEN: 1}[code]
        shapes.append((batch,) + tuple(s))
    v = [(torch.rand(s, generator=g, device=dev, dtype=torch.float32) * 2 - 1).to(tdt) for s in shapes]
    out = [torch.empty_like(t) for t in v]
    P = lambda ts: [t.data_ptr() for t in ts]
    t = alternate({
        "differential": lambda: ctx.advect_differential(grid, P(v), batch, P(v), batch, P(out)),
        "semi_lagrangian": lambda: ctx.advect_staggered(grid, P(v), P(v), P(out), 0.5),
        "laplace": lambda: ctx.field_laplace(grid, P(v), P(out), 1.0)}, reps, rounds)
    cells = batch
    for n in res:
        cells *= n
    report("advect.semi_lagrangian(v, v)", config, cells, esize, t["semi_lagrangian"], 2 * D)
    report("field.laplace(v)", config, cells, esize, t["laplace"], 2 * D)
    report("advect.differential(v, v)", config, cells, esize, t["differential"], 2 * D, {"semi_lagrangian": t["semi_lagrangian"], "laplace": t["laplace"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true", help="leave out the RK4 step against the split step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_momentum.py needs a HIP device"
    ctx = C.Context(C.load_default_library(), 0)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    staggered_group(ctx, dev, g, "256^3 f32 periodic", (256, 256, 256), 1, "f32", C.BC_PERIODIC, args.reps, args.rounds)
    staggered_group(ctx, dev, g, "384^3 f64 closed", (384, 384, 384), 1, "f64", C.BC_CLOSED, max(args.reps // 5, 5), args.rounds)
    staggered_group(ctx, dev, g, "2048^2 x 8 f32 periodic", (2048, 2048), 8, "f32", C.BC_PERIODIC, args.reps, args.rounds)
    # ---- the centred form against the centred gradient, 256^3 fp32
    n = 256
    res3 = (n, n, n)
    per = ((C.BC_PERIODIC, C.BC_PERIODIC),) * 3
    zero = [(0.0, 0.0)] * 3
    grid = C.make_grid(3, C.PHIHIP_F32, 1, res3, (0,) * 3, (float(n),) * 3, per)
    vc = torch.rand((1, 3) + res3, generator=g, device=dev) * 2 - 1
    s = torch.rand((1,) + res3, generator=g, device=dev)
    out = torch.empty_like(vc)
    t = alternate({
        "differential": lambda: ctx.advect_differential_centered(grid, vc.data_ptr(), 1, per, zero, vc.data_ptr(), 1, out.data_ptr()),
        "gradient": lambda: ctx.gradient_centered(grid, s.data_ptr(), per, zero, out.data_ptr())}, args.reps, args.rounds)
    report("gradient_centered", "256^3 f32 periodic", n ** 3, 4, t["gradient"], 4)
    report("advect.differential centred(v, v)", "256^3 f32 periodic", n ** 3, 4, t["differential"], 6, {"gradient_centered": t["gradient"]})
    del vc, s, out
    if args.skip_steps:
        return
    # ---- one RK4 step against one split step, 256^3 fp32, through the Python layer
    from phiflow_amd.flow import PERIODIC, Box, CenteredGrid, Solve, StaggeredGrid, advect, diffuse, fluid
    L = 6.283185307179586
    box = Box(x=L, y=L, z=L)
    import numpy as np
    # a rough field: fp32 CG cannot reach 1e-5 of a SMOOTH right-hand side at 256^3 (it stalls near cond * eps ~ 2e-3 of it, as a Taylor-Green start showed)
    from phiflow_amd.flow import NotConverged
    noise = StaggeredGrid([torch.rand((n, n, n), generator=g, device=dev) * 2 - 1 for _ in range(3)], PERIODIC, box, x=n, y=n, z=n)
    v0, _ = fluid.make_incompressible(noise, (), Solve('CG', 1e-5, suppress=[NotConverged]))
    p0 = CenteredGrid(0, PERIODIC, box, x=n, y=n, z=n)
    dt, nu = 0.5 * L / n, 0.01
    pde = lambda w: advect.differential(w, w) + diffuse.differential(w, nu)

    # the stage projections of the RK4 step solve for pressure INCREMENTS: their natural guess is 0. With x0 = p (the full pressure) the fp32 CG starts from a
    # residual |A p| that is orders of magnitude above the right-hand side and stagnates above 1e-5 of it; the split step solves for p itself and takes x0 = p.
    def rk4(v, p):
        return fluid.incompressible_rk4(pde, v, p, dt, pressure_order=2, pressure_solve=Solve('CG', 1e-5, suppress=[NotConverged]))

    def split(v, p):
        v = diffuse.explicit(advect.semi_lagrangian(v, v, dt), nu, dt)
        return fluid.make_incompressible(v, (), Solve('CG', 1e-5, x0=p, suppress=[NotConverged]))
    times, its, conv = {}, {}, {}
    for name, step in (("rk4", rk4), ("split", split)):
        v, p = v0, p0
        for _ in range(2):          # warm: workspaces, launch plans, a pressure guess
            v, p = step(v, p)
        best = float('inf')
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v, p = step(v, p)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        times[name] = best
        its[name] = max(p.solve_info.iterations) if p.solve_info is not None else None
        conv[name] = all(p.solve_info.converged) if p.solve_info is not None else None
    print(json.dumps({"what": "split step (semi_lagrangian + diffuse.explicit + make_incompressible)", "config": "256^3 f32 periodic, Solve('CG', 1e-5, x0=p)",
                      "ms": times["split"] * 1e3, "cg_iterations_last_solve": its["split"], "converged": conv["split"]}), flush=True)
    print(json.dumps({"what": "incompressible_rk4 step", "config": "256^3 f32 periodic, Solve('CG', 1e-5) per stage", "ms": times["rk4"] * 1e3,
                      "cg_iterations_last_solve": its["rk4"], "time_over_split_step": times["rk4"] / times["split"]}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
""" plain CG against multigrid-preconditioned CG (Solve(preconditioner='multigrid'), phihip_method 2) in ONE process, alternating:
iterations, ms per iteration, ms per solve, levels and launches of one V-cycle -- closed boxes with a solid disc / sphere (radius 0.1 of the
edge at (0.3, 0.5[, 0.5])), seeded white-noise right-hand side made mean-zero over the fluid cells, rel_tol 1e-5 from x0 = 0 and from a warm
start (x0 = the solution of a right-hand side that differs by 10 % noise: a stand-in for "the previous step's pressure").
    python tools/time_multigrid.py [--cases 128x128:1:f32,128x128x128:1:f32,...] [--rtol 1e-5] [--repeats 3] [--sweeps N --coarsest N --bottom N --omega W] """
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phiflow_amd import _capi as C   # noqa: E402

DEFAULT = "128x128:1:f32,512x512:8:f32,128x128x128:1:f32,256x256x256:1:f32,512x512x512:1:f32,384x384x384:1:f64"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT)
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, default=0)
    ap.add_argument("--coarsest", type=int, default=0)
    ap.add_argument("--bottom", type=int, default=0)
    ap.add_argument("--omega", type=float, default=0.0)
    args = ap.parse_args()
    ctx = C.Context(C.load_default_library(), 0)
    ctx.set_multigrid(args.sweeps, args.coarsest, args.bottom, args.omega)
    dev = torch.device("cuda:0")
    for spec in args.cases.split(","):
        shape_s, batch_s, dt_s = spec.split(":")
        shape, B = tuple(int(n) for n in shape_s.split("x")), int(batch_s)
        rank, dtype = len(shape), torch.float64 if dt_s == "f64" else torch.float32
        grid = C.make_grid(rank, C.PHIHIP_F64 if dt_s == "f64" else C.PHIHIP_F32, B, shape, (0,) * rank, tuple(float(n) for n in shape), ((1, 1),) * rank)
        grid1 = C.make_grid(rank, grid.dtype, 1, shape, (0,) * rank, tuple(float(n) for n in shape), ((1, 1),) * rank)
        axes = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) + 0.5 for n in shape], indexing="ij")
        centre = (0.3,) + (0.5,) * (rank - 1)
        fluid = sum((a - c * n) ** 2 for a, c, n in zip(axes, centre, shape)) > (0.1 * shape[0]) ** 2
        acc = fluid.to(torch.uint8).contiguous()
        flags = torch.empty(shape, dtype=torch.uint8, device=dev)
        ctx.build_cellflags(grid1, acc.data_ptr(), 0, 1, flags.data_ptr())
        mask = fluid.to(dtype)[None]
        gen = torch.Generator(device="cpu").manual_seed(0)

        def noise():
            r = torch.randn((B,) + shape, generator=gen, dtype=dtype).to(dev) * mask
            dims = tuple(range(1, rank + 1))
            return (r - r.sum(dim=dims, keepdim=True) / mask.sum() * mask) * mask
        rhs = noise()
        rhs_prev = rhs + 0.1 * noise()
        x = torch.zeros_like(rhs)
        warm = {}
        for method, name in ((0, "plain"), (2, "multigrid")):      # the warm start of each solver: its own solution of the neighbouring right-hand side
            w = torch.zeros_like(rhs)
            ctx.cg_solve(grid, flags.data_ptr(), 1, rhs_prev.data_ptr(), w.data_ptr(), C.Solve(args.rtol, 0.0, args.max_iterations, 50, 10, method))
            warm[name] = w
        for start in ("cold", "warm"):
            row = {"shape": shape, "batch": B, "dtype": dt_s, "rtol": args.rtol, "start": start}
            best = {"plain": None, "multigrid": None}
            for _ in range(args.repeats):
                for method, name in ((0, "plain"), (2, "multigrid")):
                    solve = C.Solve(args.rtol, 0.0, args.max_iterations, 50, 10, method)
                    if start == "cold":
                        x.zero_()
                    else:
                        x.copy_(warm[name])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    info = ctx.cg_solve(grid, flags.data_ptr(), 1, rhs.data_ptr(), x.data_ptr(), solve)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    its = max(i.iterations for i in info)
                    if best[name] is None or dt < best[name][0]:
                        best[name] = (dt, its, all(i.converged for i in info))
            for name, (dt, its, conv) in best.items():
                row[name] = {"iterations": its, "converged": conv, "ms_per_solve": round(dt * 1e3, 3), "ms_per_iteration": round(dt * 1e3 / max(its, 1), 4)}
            row["speedup"] = round(best["plain"][0] / best["multigrid"][0], 2)
            row["vcycle"] = ctx.query_multigrid()
            print(json.dumps(row), flush=True)
        del rhs, rhs_prev, x, warm, flags, acc, mask, axes, fluid
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

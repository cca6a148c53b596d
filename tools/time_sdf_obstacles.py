#!/usr/bin/env python3
"""
A moving SDF obstacle against a moving Box with the same bounding box on the MI355X (csrc/obstacle_sdf.hpp against the analytic kernels of project.hip), at
256^3 fp32 with a 64^3 and a 128^3 SDF grid. One step = what a moving obstacle costs every time step: apply_boundary_conditions (phihip_apply_obstacles)
plus the flag rebuild (phihip_obstacle_accessible + phihip_build_cellflags); the obstacle moves by a fraction of a cell per step, as in Moving_Obstacles.ipynb.
The SDF obstacles and the Box ALTERNATE in one process, best of `--rounds` rounds. The yardstick is the Box path: the parent commit's kernels, unchanged.
Before timing, the SDF path is checked on 4096 random faces and cells against a NumPy evaluation of the same grid (this size takes the second trip of the
kernels' patch loops, which the test grids do not reach). Prints one JSON line per obstacle: ms per step and the ratio to the Box. Fails without a GPU.
    python tools/time_sdf_obstacles.py [--size 256] [--reps 2000] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phiflow_amd import _capi as C   # noqa: E402


def sphere_sdf(res, lower, upper, centre, radius):
    xs = [l + (np.arange(n) + 0.5) * (u - l) / n for l, u, n in zip(lower, upper, res)]
    g = np.meshgrid(*xs, indexing='ij')
    return (np.sqrt(sum((p - c) ** 2 for p, c in zip(g, centre))) - radius).astype(np.float32)


def host_sample(vals, lower, upper, pts):
    """ multilinear, taps clamped, float64 """
    D = vals.ndim
    lo, hi, f = [], [], []
    for a in range(D):
        n = vals.shape[a]
        idx = (pts[a] - lower[a]) / (upper[a] - lower[a]) * n - 0.5
        fl = np.floor(np.clip(idx, -1, n))
        f.append(np.clip(idx, -1, n) - fl)
        lo.append(np.clip(fl.astype(np.int64), 0, n - 1))
        hi.append(np.clip(fl.astype(np.int64) + 1, 0, n - 1))
    v = vals.astype(np.float64)
    out = 0.0
    for corner in range(1 << D):
        w, index = 1.0, []
        for a in range(D):
            up = (corner >> a) & 1
            w = w * (f[a] if up else 1.0 - f[a])
            index.append(hi[a] if up else lo[a])
        out = out + w * v[tuple(index)]
    return out


def run(ctx, dev, n, reps, rounds, sync, sdf_sizes=(64, 128)):
    res = (n, n, n)
    L = float(n)
    closed = ((C.BC_CLOSED, C.BC_CLOSED),) * 3
    grid = C.make_grid(3, C.PHIHIP_F32, 1, res, (0,) * 3, (L,) * 3, closed)
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = [ctx.component_shape(grid, d) for d in range(3)]
    v0 = [torch.rand((1,) + s, generator=gen, device=dev) * 2 - 1 for s in shapes]
    v = [t.clone() for t in v0]
    acc = torch.empty(res, dtype=torch.uint8, device=dev)
    flags = torch.empty(res, dtype=torch.uint8, device=dev)
    vel = (0.3, 0.2, 0.1)
    lower0, upper0 = (0.30 * L,) * 3, (0.55 * L,) * 3            # the bounding box both obstacles share: a quarter of the domain per axis
    centre0 = tuple(0.5 * (l + u) for l, u in zip(lower0, upper0))
    radius = 0.45 * (upper0[0] - lower0[0])
    P = lambda ts: [t.data_ptr() for t in ts]
    kept = []

    def sdf_step(m):
        vals_h = sphere_sdf((m,) * 3, lower0, upper0, centre0, radius)
        vals = torch.from_numpy(vals_h).to(dev)
        kept.append(vals)
        state = {"k": 0, "slot": None}

        def step():
            k = state["k"] = (state["k"] + 1) % 8
            if state["slot"] is not None:
                ctx.sdf_release(state["slot"])
            shift = [0.05 * k * c for c in vel]
            lo, up = [l + s for l, s in zip(lower0, shift)], [u + s for u, s in zip(upper0, shift)]
            state["slot"] = ctx.sdf_bind(C.make_sdf_grid(vals.data_ptr(), C.PHIHIP_F32, (m,) * 3, lo, up, [c + s for c, s in zip(centre0, shift)], radius, True))
            arr = C.make_obstacles([dict(kind=C.OBSTACLE_SDF, slot=state["slot"], velocity=vel)])
            ctx.apply_obstacles(grid, arr, 1, P(v))
            ctx.obstacle_accessible(grid, arr, 1, acc.data_ptr())
            ctx.build_cellflags(grid, acc.data_ptr(), 0, 1, flags.data_ptr())
        return step, vals_h

    def box_step():
        state = {"k": 0}

        def step():
            k = state["k"] = (state["k"] + 1) % 8
            shift = [0.05 * k * c for c in vel]
            arr = C.make_obstacles([dict(kind=C.OBSTACLE_BOX, center=[c + s for c, s in zip(centre0, shift)], half_size=[0.5 * (u - l) for l, u in zip(lower0, upper0)],
                                         velocity=vel)])
            ctx.apply_obstacles(grid, arr, 1, P(v))
            ctx.obstacle_accessible(grid, arr, 1, acc.data_ptr())
            ctx.build_cellflags(grid, acc.data_ptr(), 0, 1, flags.data_ptr())
        return step

    # ---- check the SDF path at this size against NumPy on random samples
    rng = np.random.default_rng(0)
    for m in sdf_sizes:
        vals_h = sphere_sdf((m,) * 3, lower0, upper0, centre0, radius)
        vals = torch.from_numpy(vals_h).to(dev)
        slot = ctx.sdf_bind(C.make_sdf_grid(vals.data_ptr(), C.PHIHIP_F32, (m,) * 3, lower0, upper0, centre0, radius, True))
        arr = C.make_obstacles([dict(kind=C.OBSTACLE_SDF, slot=slot, velocity=vel)])
        w = [t.clone() for t in v0]
        ctx.apply_obstacles(grid, arr, 1, P(w))
        ctx.obstacle_accessible(grid, arr, 1, acc.data_ptr())
        sync()
        ctx.sdf_release(slot)
        cell_r = np.sqrt(0.75)
        worst = 0.0
        for d in range(3):
            shape = shapes[d]
            idx = [rng.integers(0, s, 4096) for s in shape]
            for a in range(3):          # half of the samples near the obstacle
                idx[a][:2048] = np.clip((rng.uniform(lower0[a] - 2, upper0[a] + 2, 2048)).astype(np.int64), 0, shape[a] - 1)
            pts = [idx[a] + (1.0 if a == d else 0.5) for a in range(3)]          # closed sides: stored face 0 is physical face 1
            inb = np.all([(p >= l) & (p <= u) for p, l, u in zip(pts, lower0, upper0)], axis=0)
            dist = np.where(inb, host_sample(vals_h, lower0, upper0, pts), np.sqrt(sum((p - c) ** 2 for p, c in zip(pts, centre0))) - radius)
            mask = np.clip(1.0 - dist / cell_r, 0, 1).astype(np.float32)
            old = v0[d][0][tuple(torch.from_numpy(i).to(dev) for i in idx)].cpu().numpy()
            want = np.where(mask == 1, 0, (np.float32(1) - mask) * old) + mask * np.float32(vel[d])
            got = w[d][0][tuple(torch.from_numpy(i).to(dev) for i in idx)].cpu().numpy()
            worst = max(worst, float(np.abs(got - want).max()))
        idx = [np.clip((rng.uniform(lower0[a] - 2, upper0[a] + 2, 4096)).astype(np.int64), 0, n - 1) for a in range(3)]
        pts = [i + 0.5 for i in idx]
        inb = np.all([(p >= l) & (p <= u) for p, l, u in zip(pts, lower0, upper0)], axis=0)
        val = host_sample(vals_h, lower0, upper0, pts)
        safe = np.abs(val) > 1e-6
        got = acc[tuple(torch.from_numpy(i).to(dev) for i in idx)].cpu().numpy()
        assert worst < 1e-5 and np.array_equal(got[safe], (~(inb & (val <= 0))).astype(np.uint8)[safe]), (m, worst)
        print(json.dumps({"what": "check", "sdf_res": m, "max_abs_error_4096_faces_per_component": worst, "cells_checked": int(safe.sum())}), flush=True)

    steps = {"box": box_step()}
    for m in sdf_sizes:
        steps[f"sdf{m}"] = sdf_step(m)[0]
    for fn in steps.values():
        for _ in range(3):
            fn()
    best = {k: float('inf') for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            best[k] = min(best[k], (time.perf_counter() - t0) / reps)
    for k in steps:
        line = {"what": k, "res": list(res), "dtype": "f32", "ms_per_step": best[k] * 1e3, "over_box": best[k] / best["box"]}
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_sdf_obstacles.py needs a HIP device"
    run(C.Context(C.load_default_library(), 0), torch.device("cuda:0"), args.size, args.reps, args.rounds, torch.cuda.synchronize)


if __name__ == "__main__":
    main()

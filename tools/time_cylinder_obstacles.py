#!/usr/bin/env python3
"""
What the cylinder branch of the obstacle kernels (csrc/project.hip, f16) costs on the MI355X, and whether the old kinds kept their speed.
One step = what a moving obstacle costs every time step: apply_boundary_conditions (phihip_apply_obstacles) plus the flag rebuild
(phihip_obstacle_accessible + phihip_build_cellflags); the obstacles move by a fraction of a cell per step, as in Moving_Obstacles.ipynb.
  1. `--lib PATH` (a libphihip.so of the parent commit): two boxes and a sphere at `--size`^3 fp32 through two separately loaded copies of this build's library and
     two of PATH, alternating in one process, best of `--rounds` rounds. The spread between the two copies of the same library is the margin of the comparison.
  2. a tumbling cylinder against the rotated box that circumscribes it in the same frame (the same matrix), at `--size`^3 fp32 and `--size64`^3 fp64, this build:
     a ratio, for the record.
Before timing, the cylinder path is checked at `--size` on 4096 random faces per component and 4096 cells against a NumPy evaluation (this size takes the second
trip of the kernels' patch loops, which the test grids do not reach). Prints one JSON line per measurement. Fails without a GPU.
    python tools/time_cylinder_obstacles.py [--lib parent/libphihip.so] [--size 256] [--size64 384] [--reps 1000] [--rounds 5]
"""
import argparse
import json
import math
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phiflow_amd import _capi as C   # noqa: E402

VEL = (0.3, 0.2, 0.1)
ANG = (0.02, -0.03, 0.0)


def rotation(seed=3):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def old_kinds(L, k):
    s = [0.05 * k * c for c in VEL]
    at = lambda *f: [x * L + d for x, d in zip(f, s)]
    return [dict(kind=C.OBSTACLE_BOX, center=at(0.3, 0.35, 0.4), half_size=[0.08 * L, 0.1 * L, 0.06 * L], velocity=VEL),
            dict(kind=C.OBSTACLE_BOX, center=at(0.65, 0.6, 0.55), half_size=[0.1 * L, 0.05 * L, 0.12 * L], velocity=VEL, rotation=rotation(), angular_velocity=ANG),
            dict(kind=C.OBSTACLE_SPHERE, center=at(0.5, 0.3, 0.7), half_size=[0.1 * L] * 3, velocity=VEL)]


def cylinder_item(L, k, M):
    s = [0.05 * k * c for c in VEL]
    return dict(kind=C.OBSTACLE_CYLINDER, center=[0.45 * L + d for d in s], half_size=[0.08 * L, 0.2 * L, 0.0], axis=0, rotation=M, velocity=VEL, angular_velocity=ANG)


def box_item(L, k, M):
    return dict(cylinder_item(L, k, M), kind=C.OBSTACLE_BOX, half_size=[0.2 * L, 0.08 * L, 0.08 * L], axis=0)


class Scene:
    def __init__(self, ctx, dev, n, dtype):
        self.ctx, self.res, self.L = ctx, (n, n, n), float(n)
        code = C.PHIHIP_F64 if dtype == torch.float64 else C.PHIHIP_F32
        self.grid = C.make_grid(3, code, 1, self.res, (0,) * 3, (self.L,) * 3, ((C.BC_CLOSED, C.BC_CLOSED),) * 3)
        gen = torch.Generator(device=dev).manual_seed(0)
        self.shapes = [ctx.component_shape(self.grid, d) for d in range(3)]
        self.v0 = [(torch.rand((1,) + s, generator=gen, device=dev, dtype=dtype) * 2 - 1) for s in self.shapes]
        self.v = [t.clone() for t in self.v0]
        self.acc = torch.empty(self.res, dtype=torch.uint8, device=dev)
        self.flags = torch.empty(self.res, dtype=torch.uint8, device=dev)
        self.k = 0

    def step(self, items_of, ctx=None):
        ctx = ctx or self.ctx
        self.k = (self.k + 1) % 8
        items = items_of(self.L, self.k)
        arr = C.make_obstacles(items)
        ctx.apply_obstacles(self.grid, arr, len(items), [t.data_ptr() for t in self.v])
        ctx.obstacle_accessible(self.grid, arr, len(items), self.acc.data_ptr())
        ctx.build_cellflags(self.grid, self.acc.data_ptr(), 0, 1, self.flags.data_ptr())


def check_cylinder(scene, dev, M):
    """ the cylinder path at this size against NumPy on random samples, half of them near the body """
    L, n = scene.L, scene.res[0]
    item = cylinder_item(L, 0, M)
    arr = C.make_obstacles([item])
    w = [t.clone() for t in scene.v0]
    scene.ctx.apply_obstacles(scene.grid, arr, 1, [t.data_ptr() for t in w])
    scene.ctx.obstacle_accessible(scene.grid, arr, 1, scene.acc.data_ptr())
    torch.cuda.synchronize()
    c, Rad, hd = np.asarray(item["center"]), item["half_size"][0], item["half_size"][1]

    def surfaces(pts):
        loc = M.T @ (np.stack(pts) - c[:, None])
        return np.sqrt(loc[1] ** 2 + loc[2] ** 2) - Rad, np.abs(loc[0]) - hd
    rng = np.random.default_rng(0)
    cell_r = math.sqrt(0.75)
    worst = 0.0
    near = lambda size: np.clip(rng.uniform(c[:, None] - 0.25 * L, c[:, None] + 0.25 * L, (3, size)).astype(np.int64), 0, None)
    for d in range(3):
        shape = scene.shapes[d]
        idx = [rng.integers(0, s, 4096) for s in shape]
        close = near(2048)
        for a in range(3):
            idx[a][:2048] = np.minimum(close[a], shape[a] - 1)
        pts = [idx[a] + (1.0 if a == d else 0.5) for a in range(3)]          # closed sides: stored face 0 is physical face 1
        mantle, caps = surfaces(pts)
        mask = np.clip(1.0 - np.maximum(mantle, caps) / cell_r, 0, 1).astype(np.float32)
        r = np.stack(pts) - c[:, None]
        u = np.cross(np.asarray(ANG), r.T).T[d] + VEL[d]
        at = tuple(torch.from_numpy(i).to(dev) for i in idx)
        old = scene.v0[d][0][at].cpu().numpy()
        want = np.where(mask == 1, 0, (np.float32(1) - mask) * old) + mask * np.float32(1) * u.astype(np.float32)
        worst = max(worst, float(np.abs(w[d][0][at].cpu().numpy() - want).max()))
    idx = [np.minimum(i, n - 1) for i in near(4096)]
    mantle, caps = surfaces([i + 0.5 for i in idx])
    safe = np.minimum(np.abs(mantle), np.abs(caps)) > 1e-6
    got = scene.acc[tuple(torch.from_numpy(i).to(dev) for i in idx)].cpu().numpy()
    inside = (mantle <= 0) & (caps <= 0)
    assert worst < 1e-5 and np.array_equal(got[safe], (~inside).astype(np.uint8)[safe]) and inside.sum() > 100, (worst, int(inside.sum()))
    print(json.dumps({"what": "check", "res": list(scene.res), "max_abs_error_4096_faces_per_component": worst, "cells_checked": int(safe.sum()),
                      "cells_inside": int(inside.sum())}), flush=True)


def best_of(steps, reps, rounds):
    for fn in steps.values():
        for _ in range(3):
            fn()
    best = {k: float('inf') for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            best[k] = min(best[k], (time.perf_counter() - t0) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libphihip.so of the parent commit: measurement 1")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--size64", type=int, default=384)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_cylinder_obstacles.py needs a HIP device"
    dev = torch.device("cuda:0")
    lib = C.load_default_library()
    ctx = C.Context(lib, 0)
    M = rotation(5)
    scene = Scene(ctx, dev, args.size, torch.float32)
    check_cylinder(scene, dev, M)
    if args.lib:
        tmp = tempfile.mkdtemp()
        try:
            steps = {}
            here = os.path.join(ROOT, "phiflow_amd", "lib", "libphihip.so")
            for name, src in (("this_a", here), ("parent_a", args.lib), ("this_b", here), ("parent_b", args.lib)):      # two loads of each file: separate code
                path = os.path.join(tmp, name + ".so")                                                                  # objects, separate contexts
                shutil.copy(src, path)
                steps[name] = lambda other=C.Context(C.Library(path), 0): scene.step(old_kinds, other)
            best = best_of(steps, args.reps, args.rounds)
            spread = abs(best["parent_a"] - best["parent_b"]) / min(best["parent_a"], best["parent_b"])
            this, parent = min(best["this_a"], best["this_b"]), min(best["parent_a"], best["parent_b"])
            print(json.dumps({"what": "two boxes and a sphere", "res": list(scene.res), "dtype": "f32", "ms_per_step": {k: v * 1e3 for k, v in best.items()},
                              "this_over_parent": this / parent, "parent_spread": spread, "this_spread": abs(best["this_a"] - best["this_b"]) / this,
                              "within_spread": bool(this <= max(best["parent_a"], best["parent_b"]))}), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for n, dtype, name in ((args.size, torch.float32, "f32"), (args.size64, torch.float64, "f64")):
        sc = scene if dtype == torch.float32 else Scene(ctx, dev, n, dtype)
        best = best_of({"box": lambda: sc.step(lambda L, k: [box_item(L, k, M)]), "cylinder": lambda: sc.step(lambda L, k: [cylinder_item(L, k, M)])}, args.reps, args.rounds)
        print(json.dumps({"what": "tumbling cylinder against the rotated box around it", "res": list(sc.res), "dtype": name,
                          "ms_per_step": {k: v * 1e3 for k, v in best.items()}, "cylinder_over_box": best["cylinder"] / best["box"]}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""
Centred vector fields on the MI355X (csrc/advect_cvec.hpp), in one process: the fused advection by a centred velocity (self-advection) against
the staggered self-advection of the same grid (phihip_advect_staggered, the yardstick), staggered -> centres and centred vector -> faces at
256^3, and the jit_compile'd Burgers step (examples/burgers.py) in ms per step. Prints one JSON line per measurement with us per call and the
fraction of 8 TB/s BY NEED: self-advection moves 2 C words per cell (the field in, out; the velocity is the field), a separate velocity adds D;
at_centers and the face resampling move 2 D words per cell. Fails without a GPU.
    python tools/time_centered_vector.py [--reps 50]
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


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def advection(ctx, res, dtype, batch, reps):
    dev = torch.device("cuda:0")
    tdt = torch.float64 if dtype == "f64" else torch.float32
    es = 8 if dtype == "f64" else 4
    D = len(res)
    code = C.PHIHIP_F64 if dtype == "f64" else C.PHIHIP_F32
    per = ((C.BC_PERIODIC, C.BC_PERIODIC),) * D
    grid = C.make_grid(D, code, batch, res, (0,) * D, tuple(float(n) for n in res), per)
    g = torch.Generator(device=dev).manual_seed(0)
    v = torch.rand((batch, D) + tuple(res), generator=g, device=dev, dtype=tdt) * 2 - 1      # displacements below one cell (dt = dx = 1)
    out = torch.empty_like(v)
    zero = [(0.0, 0.0)] * D
    cells = batch * int(torch.tensor(res).prod())
    t_cv = timed(lambda: ctx.advect_centered_vector(grid, v.data_ptr(), batch, D, per, zero, v.data_ptr(), batch, out.data_ptr(), 1.0), reps)
    comps = [v[:, d].contiguous() for d in range(D)]            # periodic: every component holds n faces per axis, the same bytes
    souts = [torch.empty_like(c) for c in comps]
    t_st = timed(lambda: ctx.advect_staggered(grid, [c.data_ptr() for c in comps], [c.data_ptr() for c in comps], [o.data_ptr() for o in souts], 1.0),
                 reps)
    need = 2 * D * es * cells
    return {"what": "self-advection", "res": list(res), "batch": batch, "dtype": dtype,
            "centered_us": t_cv * 1e6, "centered_of_8TBs": need / t_cv / PEAK,
            "staggered_us": t_st * 1e6, "staggered_of_8TBs": need / t_st / PEAK, "centered_over_staggered": t_cv / t_st,
            "bytes_by_need": need}


def resampling(ctx, n, reps):
    dev = torch.device("cuda:0")
    res = (n, n, n)
    per = ((C.BC_PERIODIC, C.BC_PERIODIC),) * 3
    grid = C.make_grid(3, C.PHIHIP_F32, 1, res, (0,) * 3, (float(n),) * 3, per)
    g = torch.Generator(device=dev).manual_seed(1)
    comps = [torch.rand((1,) + res, generator=g, device=dev) for _ in range(3)]
    cv = torch.empty((1, 3) + res, device=dev)
    t_c = timed(lambda: ctx.staggered_to_centered(grid, [c.data_ptr() for c in comps], cv.data_ptr()), reps)
    faces = [torch.empty_like(c) for c in comps]
    t_f = timed(lambda: ctx.centered_vector_to_staggered(grid, cv.data_ptr(), 1, per, [(0.0, 0.0)] * 3, [f.data_ptr() for f in faces]), reps)
    need = 2 * 3 * 4 * n ** 3
    return {"what": "resample", "res": list(res), "dtype": "f32", "at_centers_us": t_c * 1e6, "at_centers_of_8TBs": need / t_c / PEAK,
            "to_faces_us": t_f * 1e6, "to_faces_of_8TBs": need / t_f / PEAK, "bytes_by_need": need}


def burgers(size, steps):
    import importlib.util
    from phiflow_amd.flow import iterate, jit_compile
    spec = importlib.util.spec_from_file_location("burgers_example", os.path.join(ROOT, "examples", "burgers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    v = mod.initial_velocity(size)
    step = jit_compile(mod.step)
    v = iterate(step, 3, v)                 # capture + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = iterate(step, steps, v)
    torch.cuda.synchronize()
    return {"what": "burgers_step", "size": size, "ms_per_step": (time.perf_counter() - t0) / steps * 1e3,
            "iterations_last_step": None if v.solve_info is None else v.solve_info.iterations}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--burgers-steps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_centered_vector.py needs a HIP device"
    ctx = C.Context(C.load_default_library(), 0)
    for res, dtype, batch in (((256, 256, 256), "f32", 1), ((2048, 2048), "f32", 8), ((384, 384, 384), "f64", 1)):
        print(json.dumps(advection(ctx, res, dtype, batch, args.reps)), flush=True)
    print(json.dumps(resampling(ctx, 256, args.reps)), flush=True)
    for size in (256, 1024):
        print(json.dumps(burgers(size, args.burgers_steps)), flush=True)


if __name__ == "__main__":
    main()

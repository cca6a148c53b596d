#!/usr/bin/env python3
"""
diffuse.explicit / diffuse.implicit with a diffusivity FIELD (csrc/diffuse_coef.hpp) against the number diffusivity of the same grid, in one
process on the MI355X: one explicit call (one substep), and one implicit CG iteration (fixed iteration counts, rtol = atol = 0; the time per
iteration is the difference of two counts over their difference, so the start and the copy x0 = field drop out). Prints one JSON line per
(size, dtype) with the bytes the byte model moves / time / 8 TB/s:
    explicit  number 2 words per cell (u in, out)          field 3 words (u, a in, out)
    implicit  number ~7 words per iteration (the marching CG, stencil_march.hpp)   field 10 words (MATVEC r, d, a -> d ; UPDATE d, a, x, r -> x, r)
    python tools/time_diffuse_coef.py            (256^3 fp32 and 384^3 fp64)
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
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run(ctx, n, dtype, it_lo, it_hi, reps):
    dev = torch.device("cuda:0")
    tdt = torch.float64 if dtype == "f64" else torch.float32
    es = 8 if dtype == "f64" else 4
    codes = ((C.BC_OPEN, C.BC_OPEN),) * 3
    grid = C.make_grid(3, C.PHIHIP_F64 if dtype == "f64" else C.PHIHIP_F32, 1, (n, n, n), (0, 0, 0), (1, 1, 1), ((2, 2),) * 3)
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.rand(1, n, n, n, generator=g, device=dev, dtype=tdt)
    a = torch.rand(1, n, n, n, generator=g, device=dev, dtype=tdt) + 0.1
    out = torch.empty_like(u)
    zero = [(0.0, 0.0)] * 3
    kdt = 0.1 / n ** 2
    cells = n ** 3
    t_ex_num = timed(lambda: ctx.diffuse_explicit_centered(grid, u.data_ptr(), codes, zero, out.data_ptr(), kdt, False), reps)
    t_ex_fld = timed(lambda: ctx.diffuse_explicit_centered_coef(grid, u.data_ptr(), codes, zero, a.data_ptr(), 1, codes, zero, [kdt] * 3,
                                                                 out.data_ptr(), False), reps)
    kdt_i = 4.0 / n ** 2

    def per_iter(fn):
        lo = timed(lambda: fn(C.Solve(0.0, 0.0, it_lo, 0, 0, 0)), 2)
        hi = timed(lambda: fn(C.Solve(0.0, 0.0, it_hi, 0, 0, 0)), 2)
        return (hi - lo) / (it_hi - it_lo)
    t_im_num = per_iter(lambda s: ctx.diffuse_implicit_centered(grid, u.data_ptr(), codes, zero, out.data_ptr(), kdt_i, s, want_info=False))
    t_im_fld = per_iter(lambda s: ctx.diffuse_implicit_centered_coef(grid, u.data_ptr(), codes, zero, a.data_ptr(), 1, codes, zero, [kdt_i] * 3,
                                                                     out.data_ptr(), s, want_info=False))
    frac = lambda words, t: words * es * cells / t / PEAK
    return {"size": n, "dtype": dtype,
            "explicit_number_ms": t_ex_num * 1e3, "explicit_field_ms": t_ex_fld * 1e3, "explicit_ratio": t_ex_fld / t_ex_num,
            "explicit_number_of_8TBs": frac(2, t_ex_num), "explicit_field_of_8TBs": frac(3, t_ex_fld),
            "implicit_number_ms_per_iter": t_im_num * 1e3, "implicit_field_ms_per_iter": t_im_fld * 1e3, "implicit_ratio": t_im_fld / t_im_num,
            "implicit_number_of_8TBs": frac(7, t_im_num), "implicit_field_of_8TBs": frac(10, t_im_fld),
            "targets": {"explicit_ratio_max": 1.6, "implicit_ratio_max": 2.0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, nargs=2, default=[20, 60])
    args = ap.parse_args()
    ctx = C.Context(C.load_default_library(), 0)
    for n, dtype in ((256, "f32"), (384, "f64")):
        print(json.dumps(run(ctx, n, dtype, args.iters[0], args.iters[1], args.reps)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""
Grid differential operators on the MI355X (csrc/diffops.hpp), in one process, every pair ALTERNATING and the best of a few repetitions
(as tools/time_multigrid.py):
  laplace at 256^3 fp32                    against diffuse.explicit of the same field (both move 2 words per cell through the marching kernels)
  centred gradient, divergence at 256^3    against at_centers of a 256^3 staggered velocity (the measured neighbour-reading centred kernel, f1d)
  staggered and centred curl at 4096^2     against at_centers of the same 4096^2 velocity
Prints one JSON line per measurement: ms per call and the fraction of 8 TB/s BY NEED -- laplace 2 words per cell, gradient 1 + D, divergence
D + 1, curl 3 (2 components in, 1 out; the corner grid has (n + 1)^2 samples), at_centers 2 D. Fails without a GPU.
    python tools/time_diffops.py [--reps 300] [--rounds 5]
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


def report(what, res, t, words, ref_name, ref_rate):
    cells = 1
    for n in res:
        cells *= n
    rate = words * 4 * cells / t / PEAK
    line = {"what": what, "res": list(res), "dtype": "f32", "ms": t * 1e3, "words_per_cell": words, "of_8TBs_by_need": rate}
    if ref_name:
        line[f"rate_over_{ref_name}"] = rate / ref_rate
    print(json.dumps(line), flush=True)
    return rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_diffops.py needs a HIP device"
    ctx = C.Context(C.load_default_library(), 0)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def rand(*shape):
        return torch.rand(shape, generator=g, device=dev) * 2 - 1
    P = lambda ts: [t.data_ptr() for t in ts]
    # ---- 256^3: the calls go through the C ABI (the host cost of the Python layer would be a third of these kernels' time)
    n = 256
    res3 = (n, n, n)
    per = ((C.BC_PERIODIC, C.BC_PERIODIC),) * 3
    zero = [(0.0, 0.0)] * 3
    grid = C.make_grid(3, C.PHIHIP_F32, 1, res3, (0,) * 3, (float(n),) * 3, per)
    s, out = rand(1, *res3), torch.empty((1,) + res3, device=dev)
    vc, gout = rand(1, 3, *res3), torch.empty((1, 3) + res3, device=dev)
    comps = [rand(1, *res3) for _ in range(3)]
    t = alternate({
        "laplace": lambda: ctx.field_laplace_centered(grid, s.data_ptr(), per, zero, [1.0, 1.0, 1.0], out.data_ptr()),
        "diffuse": lambda: ctx.diffuse_explicit_centered(grid, s.data_ptr(), per, zero, out.data_ptr(), 0.1),
        "gradient": lambda: ctx.gradient_centered(grid, s.data_ptr(), per, zero, gout.data_ptr()),
        "divergence": lambda: ctx.divergence_centered(grid, vc.data_ptr(), per, zero, out.data_ptr()),
        "at_centers": lambda: ctx.staggered_to_centered(grid, P(comps), gout.data_ptr())}, args.reps, args.rounds)
    r_diff = report("diffuse.explicit", res3, t["diffuse"], 2, None, None)
    report("laplace", res3, t["laplace"], 2, "diffuse", r_diff)
    r_c = report("at_centers", res3, t["at_centers"], 6, None, None)
    report("gradient_centered", res3, t["gradient"], 4, "at_centers", r_c)
    report("divergence_centered", res3, t["divergence"], 4, "at_centers", r_c)
    del s, out, vc, gout, comps
    # ---- 4096^2
    m = 4096
    res2 = (m, m)
    grid2 = C.make_grid(2, C.PHIHIP_F32, 1, res2, (0,) * 2, (float(m),) * 2, per[:2])
    vx, vy = rand(1, m + 1, m), rand(1, m, m + 1)           # all faces, as Field.curl bakes them
    v2c, corners = rand(1, 2, m, m), torch.empty((1, m + 1, m + 1), device=dev)
    comps2, cv2 = [rand(1, m, m) for _ in range(2)], torch.empty((1, 2, m, m), device=dev)
    t = alternate({
        "curl_staggered": lambda: ctx.curl_2d(grid2, True, vx.data_ptr(), vy.data_ptr(), per[:2], zero[:2], corners.data_ptr()),
        "curl_centred": lambda: ctx.curl_2d(grid2, False, v2c.data_ptr(), 0, per[:2], zero[:2], corners.data_ptr()),
        "at_centers": lambda: ctx.staggered_to_centered(grid2, P(comps2), cv2.data_ptr())}, args.reps, args.rounds)
    r_c = report("at_centers", res2, t["at_centers"], 4, None, None)
    report("curl_staggered", res2, t["curl_staggered"], 3, "at_centers", r_c)
    report("curl_centred", res2, t["curl_centred"], 3, "at_centers", r_c)


if __name__ == "__main__":
    main()

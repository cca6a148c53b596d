#!/usr/bin/env python3
"""
Randomised parity run: random resolutions (degenerate ones included), boundary mixes, wall velocities, batch sizes and dtypes through
every check of tests/parity_cases.py (kernels vs the NumPy oracle), on the GPU library or on the CPU emulation build.
  python tests/fuzz_parity.py --first 0 --count 100 [--emu]
Prints one line per case; exit code 1 if any case failed. Known limitation that is reported as "skip": an axis with ONE cell between
two closed sides has no stored faces.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # this file lives there: test infrastructure (it drives the oracle)
import adjoint_cases as ac           # noqa: E402
import advect_forward_cases as afc   # noqa: E402
import diffuse_coef_elementwise_cases as dce   # noqa: E402
import multigrid_elementwise_cases as mgc   # noqa: E402
import parity_cases as pc            # noqa: E402
import project_elementwise_cases as pec   # noqa: E402
import slab_phase_cases as spc       # noqa: E402
from phiflow_amd import _capi as C   # noqa: E402


def resident_arm(ctx, mem, r, seed, bc, emu):
    """ r5: the opt-in resident solver (cg_resident.hip: the whole 2-D fp32 solve as ONE launch, paired 16-byte `sc1`
    granules) on a random eligible grid with this case's boundary mix -- rows of whole vectors up to 512 cells, a ragged last workgroup more
    often than not, batch x workgroups <= CUs: fixed iterations across a true-residual refresh, tolerance mode, the balanced projection. The
    launch counters assert that the resident kernel is what ran (one launch, no MATVEC launches). """
    n2 = 4 * int(r.integers(2, 20 if emu else 129))
    n1 = int(r.integers(2, 60 if emu else 400))
    G = (n1 + 15) // 16
    batch = int(r.integers(1, max(2, min(9, (16 if emu else 256) // G + 1))))
    dom, grid = pc.make_case((n1, n2), bc, np.float32, batch=batch)
    try:
        ctx.set_resident_cg(2)
        ctx.profile_enable(True)
        ctx.profile_read(True)
        pc.check_cg(ctx, mem, dom, grid, np.float32, np.random.default_rng(seed + 7), max_iter=int(r.integers(3, 40)), refresh=int(r.integers(2, 12)),
                    fixed_iterations=True)
        prof = ctx.profile_read(True)
        assert prof["cg_matvec_dot"][0] == 0 and prof["cg_update"][0] == 1, f"the resident solver did not run ({n1} x {n2} x {batch}): {prof}"
        ctx.profile_enable(False)
        if n1 * n2 <= 40000:      # tolerance mode on a white-noise right-hand side: thousands of iterations on larger 2-D grids (max_iterations = 1000)
            pc.check_cg(ctx, mem, dom, grid, np.float32, np.random.default_rng(seed + 8))
            pc.check_make_incompressible(ctx, mem, dom, grid, np.float32, np.random.default_rng(seed + 9))
        if 8192 < n1 * n2 <= 40000:      # r6: the FLAGS form of the resident solver -- a random solid disc (below 8193 cells the one-workgroup solver takes a solve)
            rad = float(r.uniform(0.12, 0.3)) * min(n1, n2)
            disc = pc.O.SphereObstacle((float(r.uniform(0.3, 0.7)) * n1, float(r.uniform(0.3, 0.7)) * n2), rad)
            pc.check_resident_with_flags(ctx, mem, (n1, n2), bc, batch, [disc], seed=seed + 10, projection=not all(lo == pc.PER for lo, _ in bc))
    finally:
        ctx.profile_enable(False)
        ctx.set_resident_cg(1)          # the library's default since r6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=50)
    ap.add_argument("--emu", action="store_true", help="CPU emulation build (tests/hipemu) instead of the GPU library")
    ap.add_argument("--max-res", type=int, default=0, help="largest resolution per axis (default: 22 in 2-D, 11 in 3-D; GPU: 48 / 20)")
    args = ap.parse_args()
    if args.emu:
        ctx = C.Context(C.Library(os.environ.get("PHIHIP_EMU_LIB", os.path.join(ROOT, "tests", "hipemu", "libphihip_emu.so"))), 0)
        mem = pc.NumpyMem()
    else:
        ctx = C.Context(C.load_default_library(), 0)
        mem = pc.TorchMem()
    PER, CLO, OPN = pc.PER, pc.CLO, pc.OPN
    ranks = [C.Context(ctx.lib, 0) for _ in range(3)]      # the emulated ranks of the slab-decomposed CG phases
    for c in ranks:
        c.set_autotune(False)
    fails = 0
    for seed in range(args.first, args.first + args.count):
        r = np.random.default_rng(seed)
        D = int(r.integers(2, 4))
        hi = args.max_res or ((22 if D == 2 else 11) if args.emu else (48 if D == 2 else 20))
        res = tuple(int(x) for x in r.integers(1, hi, D))
        if r.random() < 0.3:
            res = res[:-1] + (int(r.choice([4, 8, 12, 16, 64, 68])),)   # vector path of the marching kernels
        bc = tuple((PER, PER) if r.integers(0, 4) == 0 else (int(r.choice([CLO, OPN])), int(r.choice([CLO, OPN]))) for _ in range(D))
        dtype = np.float32 if r.random() < 0.5 else np.float64
        batch = int(r.integers(1, 4))
        bcv = None
        if r.random() < 0.4:
            bcv = [[[float(r.normal()) * 0.3 if bc[a][s] == CLO else 0.0 for c in range(D)] for s in range(2)] for a in range(D)]
            for a in range(D):      # no flow through the walls (a closed box with net inflow has no divergence-free solution)
                for s in range(2):
                    bcv[a][s][a] = 0.0
        tag = f"seed={seed} res={res} bc={bc} {dtype.__name__} B={batch} bcv={'y' if bcv else 'n'}"
        if any(n == 1 and b == (CLO, CLO) for n, b in zip(res, bc)):
            print("skip", tag, flush=True)
            continue
        step = "setup"
        try:
            dom, grid = pc.make_case(res, bc, dtype, batch=batch, bc_val=bcv)
            rng = np.random.default_rng(seed + 1000)
            s_codes = tuple((PER, PER) if lo == PER else (int(r.choice([CLO, OPN])), int(r.choice([CLO, OPN]))) for lo, _ in bc)
            s_consts = [(float(r.normal()), 0.25)] * D
            step = "laplace"; pc.check_laplace(ctx, mem, dom, grid, dtype, rng)
            step = "divergence"; pc.check_divergence(ctx, mem, dom, grid, dtype, rng, balance=not dom.flexible())
            step = "grad_subtract"; pc.check_grad_subtract(ctx, mem, dom, grid, dtype, rng)
            if all(n >= 4 for n in res):
                step = "grad_subtract_flags"; pc.check_grad_subtract_flags(ctx, mem, dom, grid, dtype, rng)
            step = "advect_staggered"; pc.check_advect_staggered(ctx, mem, dom, grid, dtype, rng, dt=float(r.uniform(0.1, 3.0)))
            step = "advect_centered"; pc.check_advect_centered(ctx, mem, dom, grid, dtype, rng, s_codes, s_consts)
            step = "mac_cormack_centered"
            pc.check_mac_cormack_centered(ctx, mem, dom, grid, dtype, rng, s_codes, s_consts, dt=float(r.uniform(0.1, 2.5)), strength=float(r.uniform(0.3, 1)))
            step = "mac_cormack_staggered"; pc.check_mac_cormack_staggered(ctx, mem, dom, grid, dtype, rng)
            step = "centered_to_staggered"; pc.check_centered_to_staggered(ctx, mem, dom, grid, dtype, rng, s_codes, s_consts)
            step = "diffuse"; pc.check_diffuse(ctx, mem, dom, grid, dtype, rng)
            step = "diffuse_implicit"; pc.check_diffuse_implicit(ctx, mem, dom, grid, dtype, rng, s_codes, s_consts)
            step = "grid_sample"; pc.check_grid_sample(ctx, mem, res, s_codes, [c for c in s_consts], dtype, rng, batch=batch, points=97)
            for small in (True, False):
                ctx.set_small_grid_solver(small)
                step = f"cg small={small}"; pc.check_cg(ctx, mem, dom, grid, dtype, np.random.default_rng(seed))
                step = f"cg adaptive small={small}"; pc.check_cg(ctx, mem, dom, grid, dtype, np.random.default_rng(seed), refresh=20, adaptive=True)
                step = f"make_incompressible small={small}"; pc.check_make_incompressible(ctx, mem, dom, grid, dtype, np.random.default_rng(seed + 5))
            ctx.set_small_grid_solver(True)
            if D == 2:
                step = "resident cg"; resident_arm(ctx, mem, r, seed, bc, args.emu)
            if dtype == np.float64 and min(res) >= 2:
                step = "project_backward"; pc.check_project_backward(ctx, mem, dom, grid, rng)
                step = "advect_backward"; pc.check_advect_backward(ctx, mem, dom, grid, rng, s_codes, s_consts, dt=float(r.uniform(0.1, 1.5)))
            # element by element against torch.autograd through the float64 restatement (tests/adjoint_cases.py), in BOTH element types whatever the case's own
            # is: the checks build their own velocities and wall values on the case's grid and boundary mix
            adt = float(r.uniform(0.1, 3.0))
            for edt in (np.float32, np.float64):
                step = f"adjoint elementwise staggered {edt.__name__}"
                ac.check_advect_staggered(ctx, mem, res, bc, edt, batch, adt, seed=seed, k0=int(r.integers(-1, 1)), slab_axis=int(r.integers(0, D)))
                step = f"adjoint elementwise centred {edt.__name__}"
                ac.check_advect_centered(ctx, mem, res, bc, edt, batch, adt, seed=seed, k0=int(r.integers(-1, 1)), slab_axis=int(r.integers(0, D)), flip=bool(r.integers(0, 2)))
            # the forward passes element by element under the per-sample bound of tests/advect_forward_cases.py, on every path, in BOTH element types: the
            # checks build their own fields and wall values on the case's grid and boundary mix
            fst = float(r.uniform(0.3, 1))
            for edt in (np.float32, np.float64):
                for entry in afc.ENTRIES:
                    step = f"advect forward elementwise {entry} {edt.__name__}"
                    afc.check_entry(ctx, mem, entry, res, bc, edt, batch, adt, "random", seed=seed, strength=fst)
            del afc.RECORDS[:]
            # one multigrid V-cycle element by element against the float64 restatement of its recipe (tests/multigrid_ref.py) in fp64, whatever the case's
            # element type: this case's grid and walls, random cell sizes, a random solid sphere more often than not (a PERIODIC axis of one cell is outside
            # what the reference restates)
            if not any(n == 1 and b == (PER, PER) for n, b in zip(res, bc)):
                step = "multigrid cycle elementwise"
                upper = tuple(float(n * r.uniform(0.3, 2.0)) for n in res)
                ball = (tuple(float(r.uniform(0.2, 0.8)) * u for u in upper), float(r.uniform(0.1, 0.3)) * min(upper)) if r.random() < 0.7 else None
                mgc.check_cycle_random(ctx, mem, res, bc, upper, ball, seed)
            # the first three iterations of diffuse.implicit's CG with a coefficient field, element by element against the float64 restatement
            # (tests/diffuse_coef_ref.py) in fp64, whatever the case's element type: this case's grid and scalar walls, a refresh on the second iteration
            step = "diffuse coef trajectory elementwise"
            dce.check_cg_trajectory_random(ctx, mem, res, s_codes, seed)
            # the projection stencils and the obstacle kernels element by element under the per-sample bound of tests/project_elementwise_cases.py, in BOTH
            # element types: the checks build their own fields on the case's grid and boundary mix, with every wall constant non-zero (the normal ones included)
            mode = pec.MODES[int(r.integers(0, 3))]
            for edt in (np.float32, np.float64):
                for kind in ("random", "graded"):
                    step = f"project elementwise divergence {edt.__name__}"
                    pec.check_divergence(ctx, mem, res, bc, edt, batch, kind, "none", seed)
                    pec.check_divergence(ctx, mem, res, bc, edt, batch, kind, mode, seed)
                    step = f"project elementwise grad_subtract {edt.__name__}"; pec.check_grad_subtract(ctx, mem, res, bc, edt, batch, kind, mode, seed)
                    step = f"project elementwise laplace {edt.__name__}"; pec.check_laplace(ctx, mem, res, bc, edt, batch, kind, mode, seed)
                step = f"project elementwise resample {edt.__name__}"; pec.check_centered_to_staggered(ctx, mem, res, bc, edt, batch, "random", seed, rotations=(seed % 4,))
                step = f"project elementwise diffuse {edt.__name__}"; pec.check_diffuse_explicit(ctx, mem, res, bc, edt, batch, "random", seed)
                step = f"project elementwise obstacles {edt.__name__}"
                pdx = pec.make_inputs(res, bc, edt, batch).dx
                for name in ("rotated box", "sphere", "union of three"):
                    pec.check_obstacles(ctx, mem, res, bc, edt, batch, pec.pick_scene(name, res, bc, pdx, seed), "random", seed, what=name)
            # the slab-decomposed CG phases element by element under the bounds of tests/slab_phase_cases.py: a 3-D grid of its own cut at one or two random
            # planes, a random slab-axis boundary pair, flags across the cuts or none, in the case's element type
            step = "slab phases elementwise"
            sres = (int(r.integers(3, 9)), int(r.integers(3, 7)), int(r.integers(7, 21)))
            scuts = sorted(int(c) for c in r.choice(np.arange(1, sres[0]), size=int(r.integers(1, 3)), replace=False))
            sbc = (spc.SLAB_BCS[int(r.integers(0, 3))],) + tuple(spc.KINDS[int(k)] for k in r.integers(0, 5, 2))
            spc.phases(spc.World(ranks, mem, sres, sbc, dtype, [0] + scuts + [sres[0]], "random", bool(r.integers(0, 2)), seed))
            del pec.RECORDS[:]
            print("ok  ", tag, flush=True)
        except Exception as e:   # noqa: BLE001 -- report and go on
            fails += 1
            ctx.set_small_grid_solver(True)
            print("FAIL", tag, step, type(e).__name__, str(e)[:240].replace("\n", " "), flush=True)
            if os.environ.get("FUZZ_TRACE"):
                import traceback
                traceback.print_exc()
    print("fails", fails)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())

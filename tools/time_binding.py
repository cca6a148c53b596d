#!/usr/bin/env python3
"""
Host cost of the ctypes binding (phiflow_amd/_capi.py) of one or more source trees, without a GPU: import of the module, construction of
`Library` on the emulation library (tests/hipemu/libphihip_emu.so of THIS tree) and the time per call of a few `Context` wrappers over a
stand-in library whose entry points are Python callables that return 0. One process per tree and round, the trees alternating:
    python tools/time_binding.py --trees /path/to/parent . --rounds 5 >> profiles/f17_binding_cpu.jsonl
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_LIB = os.path.join(ROOT, "tests", "hipemu", "libphihip_emu.so")


def measure(tree: str, calls: int) -> dict:
    import ctypes, re  # noqa: E401,F401  (what _capi imports itself is not part of its import time)
    import torch  # noqa: F401  (Library.__init__ imports it)
    sys.path.insert(0, tree)
    t0 = time.perf_counter()
    from phiflow_amd import _capi as C
    rec = {"tree": tree, "import_ms": (time.perf_counter() - t0) * 1e3}
    t0 = time.perf_counter()
    C.Library(EMU_LIB)
    rec["library_first_ms"] = (time.perf_counter() - t0) * 1e3      # (includes dlopen)
    best = float("inf")
    for _ in range(20):
        t0 = time.perf_counter()
        C.Library(EMU_LIB)
        best = min(best, time.perf_counter() - t0)
    rec["library_ms"] = best * 1e3

    class Dll:
        def __getattr__(self, name):
            fn = lambda *a: 0   # noqa: E731
            self.__dict__[name] = fn
            return fn
    lib = C.Library.__new__(C.Library)
    lib.dll = Dll()
    ctx = C.Context(lib, 0)
    grid = C.make_grid(3, C.PHIHIP_F32, 2, (8, 8, 8), (0, 0, 0), (1, 1, 1), ((C.BC_CLOSED, C.BC_CLOSED),) * 3)
    solve = C.Solve(1e-5, 0.0, 100, 50, 10, 0)
    p3, bc, val = [4096, 8192, 12288], ((C.BC_OPEN, C.BC_OPEN),) * 3, ((0.0, 0.0),) * 3
    cases = {
        "advect_staggered": lambda: ctx.advect_staggered(grid, p3, p3, p3, 0.1),
        "mac_cormack_centered": lambda: ctx.mac_cormack_centered(grid, 64, bc, val, p3, 128, 0.1),
        "make_incompressible": lambda: ctx.make_incompressible(grid, p3, None, 0, 1, 1, 64, 0, solve, want_info=False),
        "make_incompressible_info": lambda: ctx.make_incompressible(grid, p3, None, 0, 1, 1, 64, 0, solve, want_info=True),
        "diffuse_explicit_centered_coef": lambda: ctx.diffuse_explicit_centered_coef(grid, 64, bc, val, 0, 1, bc, val, (0.1, 0.1, 0.1), 128),
        "slab_matvec": lambda: ctx.slab_matvec(grid, (1, 0), 0, True, 64, 128, (192, 0), 256, (320, 0), 384, 448, solve),
        "set_tuning": lambda: ctx.set_tuning(1, 64, 4),
    }
    for name, fn in cases.items():
        best = float("inf")
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            best = min(best, time.perf_counter() - t0)
        rec[name + "_us"] = best / calls * 1e6
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", nargs="+", default=[ROOT])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--worker", default=None, help="(internal) measure this tree in this process")
    args = ap.parse_args()
    if args.worker:
        print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in measure(args.worker, args.calls).items()}))
        return
    for rnd in range(args.rounds):
        for tree in args.trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.abspath(tree), "--calls", str(args.calls)],
                                 check=True, capture_output=True, text=True).stdout
            print(json.dumps({"round": rnd, **json.loads(out.strip().splitlines()[-1])}), flush=True)


if __name__ == "__main__":
    main()

"""
TEST HELPER (run as a subprocess by tests/test_adjoint_elementwise_emu.py and tests/test_gpu_adjoint_elementwise.py): one element-wise case per adjoint
entry point (tests/adjoint_cases.py) in a process whose environment chooses the launch form of the staggered adjoints (PHIHIP_ADJOINT_ALL: the library
reads it once). tests/test_adjoint_forms.py asserts that both forms give the same bits; this asserts that the per-component form is CORRECT.
    python tests/adjoint_elementwise_probe.py emu|gpu
Exit status 0: every check passed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adjoint_cases as A          # noqa: E402
import parity_cases as pc          # noqa: E402
from phiflow_amd import _capi      # noqa: E402


def main():
    where = sys.argv[1]
    if where == "emu":
        os.environ["PHIHIP_AUTOTUNE"] = "0"
        lib = _capi.Library(os.environ.get("PHIHIP_EMU_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu", "libphihip_emu.so")))
        mem = pc.NumpyMem()
    else:
        lib = _capi.load_default_library()
        mem = pc.TorchMem()
    ctx = _capi.Context(lib, 0)
    print("PHIHIP_ADJOINT_ALL =", os.environ.get("PHIHIP_ADJOINT_ALL"), flush=True)
    A.run_case(ctx, mem, (9, 17, 66), A.MIX3[0], np.float32, batch=1, dt=0.7, seed=3, k0=0, slab_axis=2)
    A.run_case(ctx, mem, (5, 9, 33), A.MIX3[1], np.float64, batch=2, dt=0.7, seed=3)
    A.run_case(ctx, mem, (8, 32), A.MIX2[1], np.float64, batch=2, dt=2.9, seed=3)
    A.run_case(ctx, mem, (17, 65), A.MIX2[3], np.float32, batch=2, dt=0.7, seed=3, k0=-1, slab_axis=0, flip=True)
    A.run_grid_sample(ctx, mem, (5, 4, 9), A.GRID_SAMPLE_CASES[2][1], np.float32, False)
    print("probe ok", flush=True)


if __name__ == "__main__":
    main()

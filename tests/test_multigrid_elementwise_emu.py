"""
The multigrid V-cycle and the preconditioned CG loop of csrc/multigrid.hpp, ELEMENT BY ELEMENT against the float64 restatement of the documented recipe
(tests/multigrid_ref.py), on the emulation library. The checks, the case table and the bounds are in tests/multigrid_elementwise_cases.py;
tests/test_gpu_multigrid_elementwise.py runs the same table on the MI355X. Every case prints its measured errors before it asserts.
"""
import numpy as np
import pytest

import multigrid_elementwise_cases as E
from parity_cases import NumpyMem
from phiflow_amd import _capi

MEM = NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture()
def own_ctx(emu_library):
    """ a context of its own for what changes the V-cycle's parameters (emu_ctx is shared by the session) """
    ctx = _capi.Context(emu_library, 0)
    yield ctx
    ctx.close()


@DTYPES
@pytest.mark.parametrize("name", E.SMALL)
def test_cycle_equals_the_reference(emu_ctx, name, dtype):
    E.check_cycle(emu_ctx, MEM, name, dtype)


@DTYPES
@pytest.mark.parametrize("name,params", E.PARAMETERS, ids=[f"{n}-{'-'.join(str(v) for v in p)}" for n, p in E.PARAMETERS])
def test_cycle_with_other_parameters_equals_the_reference(own_ctx, name, params, dtype):
    E.check_cycle(own_ctx, MEM, name, dtype, params)
    assert own_ctx.query_multigrid()["levels"] == E.reference(name, params[1]).nlevels


def test_cycle_above_524288_cells_equals_the_reference(emu_ctx):
    """ (724, 726) in fp64: every workgroup's chunk of cells is larger than the workgroup. The other case above kMgBlocks * kBlock cells, (96, 80, 72),
    and fp32 run on the GPU only (about 9 s each here) """
    E.check_cycle(emu_ctx, MEM, 'large_2d', np.float64)


@pytest.mark.parametrize("name", E.IMPULSE_CASES)
def test_columns_of_the_cycle_equal_the_reference(emu_ctx, name):
    E.check_impulses(emu_ctx, MEM, name)


@DTYPES
@pytest.mark.parametrize("name", list(E.BATCH_CASES))
def test_batched_geometries_equal_their_own_reference_and_the_single_calls(emu_ctx, name, dtype):
    E.check_batch(emu_ctx, MEM, name, dtype)


@DTYPES
@pytest.mark.parametrize("K,refresh_every", E.TRAJECTORIES)
@pytest.mark.parametrize("name", E.TRAJECTORY_CASES)
def test_first_iterations_of_the_preconditioned_cg_equal_the_reference(emu_ctx, name, K, refresh_every, dtype):
    E.check_pcg_trajectory(emu_ctx, MEM, name, dtype, K, refresh_every)


def test_the_reference_imports_nothing_under_test():
    import ast
    import multigrid_ref
    tree = ast.parse(open(multigrid_ref.__file__).read())
    names = [n.module or '' for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert not [m for m in names if m.split('.')[0] == 'phiflow_amd'], names

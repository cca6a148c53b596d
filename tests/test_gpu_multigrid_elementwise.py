"""
`-m gpu`: the multigrid V-cycle and the preconditioned CG loop of csrc/multigrid.hpp on the MI355X, ELEMENT BY ELEMENT against the float64 restatement of the
documented recipe (tests/multigrid_ref.py): the table of tests/test_multigrid_elementwise_emu.py plus the two grids above kMgBlocks * kBlock = 524 288 cells,
where mg_range hands a workgroup more cells than it has threads and xcd_order decides which. Checks, cases and bounds: tests/multigrid_elementwise_cases.py.
One process; what changes the V-cycle's parameters restores the defaults. Every case prints its measured errors before it asserts.
"""
import numpy as np
import pytest

import multigrid_elementwise_cases as E
import parity_cases as pc

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("name", E.SMALL)
def test_cycle_equals_the_reference(ctx, mem, name, dtype):
    E.check_cycle(ctx, mem, name, dtype)


@DTYPES
@pytest.mark.parametrize("name,params", E.PARAMETERS, ids=[f"{n}-{'-'.join(str(v) for v in p)}" for n, p in E.PARAMETERS])
def test_cycle_with_other_parameters_equals_the_reference(ctx, mem, name, params, dtype):
    try:
        E.check_cycle(ctx, mem, name, dtype, params)
    finally:
        ctx.set_multigrid(*E.DEFAULTS)


@DTYPES
@pytest.mark.parametrize("name", E.LARGE)
def test_cycle_above_524288_cells_equals_the_reference(ctx, mem, name, dtype):
    E.check_cycle(ctx, mem, name, dtype)


@pytest.mark.parametrize("name", E.IMPULSE_CASES)
def test_columns_of_the_cycle_equal_the_reference(ctx, mem, name):
    E.check_impulses(ctx, mem, name)


@DTYPES
@pytest.mark.parametrize("name", list(E.BATCH_CASES))
def test_batched_geometries_equal_their_own_reference_and_the_single_calls(ctx, mem, name, dtype):
    E.check_batch(ctx, mem, name, dtype)


@DTYPES
@pytest.mark.parametrize("K,refresh_every", E.TRAJECTORIES)
@pytest.mark.parametrize("name", E.TRAJECTORY_CASES)
def test_first_iterations_of_the_preconditioned_cg_equal_the_reference(ctx, mem, name, K, refresh_every, dtype):
    E.check_pcg_trajectory(ctx, mem, name, dtype, K, refresh_every)

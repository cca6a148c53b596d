"""
`-m gpu`: diffusion with a varying / per-axis diffusivity (phiflow_amd/csrc/diffuse_coef.hpp) on the MI355X, ELEMENT BY ELEMENT against the float64 restatement
of tests/diffuse_coef_ref.py: the tables of tests/test_diffuse_coef_elementwise_emu.py plus the grids on which a workgroup marches several a0 planes with a
ragged last chunk -- (115, 33, 65) under the CG's plan, (231, 33, 65) under the explicit pass's -- and one mid-size grid. Checks, cases and bounds:
tests/diffuse_coef_elementwise_cases.py. One process. Every case prints its measured errors before it asserts.
"""
import numpy as np
import pytest

import diffuse_coef_elementwise_cases as E
import parity_cases as pc

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
METHODS = pytest.mark.parametrize("method", ['CG', 'CG-adaptive'])
_ids = lambda cases: [c.id for c in cases]
_tid = lambda t: f"K{t[0]}-refresh{t[1]}-{t[2]}"


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("case", E.TABLE + E.NON_AFFINE + E.FULL, ids=_ids(E.TABLE + E.NON_AFFINE + E.FULL))
def test_explicit_step_equals_the_reference(ctx, mem, case, dtype):
    E.check_explicit(ctx, mem, case, dtype)


@DTYPES
@pytest.mark.parametrize("case", E.TABLE, ids=_ids(E.TABLE))
def test_first_iterations_of_the_cg_equal_the_reference(ctx, mem, case, dtype):
    E.check_cg_trajectory(ctx, mem, case, dtype)


@DTYPES
@pytest.mark.parametrize("trajectory", E.TRAJECTORIES, ids=_tid)
@pytest.mark.parametrize("case", E.FULL, ids=_ids(E.FULL))
def test_every_trajectory_setting_equals_the_reference(ctx, mem, case, trajectory, dtype):
    E.check_cg_trajectory(ctx, mem, case, dtype, *trajectory)


@DTYPES
@pytest.mark.parametrize("trajectory", [E.TRAJECTORIES[1], E.TRAJECTORIES[4]], ids=_tid)
@pytest.mark.parametrize("case", E.NON_AFFINE, ids=_ids(E.NON_AFFINE))
def test_first_iterations_without_constant_walls_equal_the_reference(ctx, mem, case, trajectory, dtype):
    E.check_cg_trajectory(ctx, mem, case, dtype, *trajectory)


@DTYPES
@pytest.mark.parametrize("trajectory", E.CHUNKED_TRAJECTORIES, ids=_tid)
@pytest.mark.parametrize("walls", list(E.CHUNKED_CG))
def test_cg_marching_three_planes_per_workgroup_equals_the_reference(ctx, mem, walls, trajectory, dtype):
    """ (115, 33, 65): chunk 3, 39 chunks, one plane in the last; the register rotation across chunk boundaries, the clip of the last chunk, the a0 wrap into
    another workgroup's chunk and the coefficient's ghost rules on a0 """
    E.check_cg_trajectory(ctx, mem, E.CHUNKED_CG[walls], dtype, *trajectory)


@DTYPES
@pytest.mark.parametrize("walls", list(E.CHUNKED_EXPLICIT))
def test_explicit_step_marching_two_planes_per_workgroup_equals_the_reference(ctx, mem, walls, dtype):
    """ (231, 33, 65): chunk 2, 116 chunks, one plane in the last """
    E.check_explicit(ctx, mem, E.CHUNKED_EXPLICIT[walls], dtype, forms=('shared', 'absent'))


def test_mid_size_grid_equals_the_reference(ctx, mem):
    """ (64, 66, 130) in fp32: 51 tiles, ragged on both in-plane axes, four planes per workgroup in the CG """
    E.check_explicit(ctx, mem, E.MID, np.float32, forms=('shared',))
    E.check_cg_trajectory(ctx, mem, E.MID, np.float32, 4, 50, 'CG')


@DTYPES
@METHODS
@pytest.mark.parametrize("check_every", [1, 10])
def test_batch_entries_that_stop_at_different_iterations(ctx, mem, method, check_every, dtype):
    """ (on the device a solve takes milliseconds: every combination is polled every tenth iteration too) """
    E.check_batch_freeze(ctx, mem, dtype, method, check_every)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ['mixed3d', 'heat_flow', 'constants2d'])
def test_python_extrapolations_against_literal_wall_tables(gpu_backend, name, bits):
    E.check_python_walls(gpu_backend, name, bits)

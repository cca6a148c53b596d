"""
`-m gpu`: element-wise parity of the projection stencils and obstacle kernels on the MI355X, in fp32 and fp64 -- the tables of
tests/test_project_elementwise_emu.py through device memory, and the groups that take the emulation too long: several planes per workgroup of the divergence
((4099, 3, 5) scalar, (4099, 2, 8) vector), the second trip of grad_subtract's patch loop ((16 400, 3, 8), (16 400, 3, 5)) and of the balance loops ((130, 130, 130)).
Reference and comparison rule: tests/project_elementwise_cases.py. Every case prints its figures.
"""
import numpy as np
import pytest

import adjoint_cases as A
import parity_cases as pc
import project_elementwise_cases as P

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SMALL = A.SMALL_CASES[::2]
_id = P.case_id
_DT = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("case", P.ROW_CASES, ids=_id)
def test_rows_and_vectors(ctx, mem, case, dtype):
    P.run_stencils(ctx, mem, case[0], case[1], dtype, case[2], seed=1)


@DTYPES
@pytest.mark.parametrize("case", SMALL, ids=A.case_id)
def test_axes_of_one_to_three_cells(ctx, mem, case, dtype):
    P.run_stencils(ctx, mem, case[0], case[1], dtype, case[2], kinds=("random", "tiny", "nonfinite"), seed=2)


@DTYPES
@pytest.mark.parametrize("case", P.UNALIGNED_CASES, ids=_id)
def test_scalar_kernels_on_whole_vector_rows(ctx, mem, case, dtype):
    P.run_stencils(ctx, mem, case[0], case[1], dtype, case[2], kinds=("random", "graded"), seed=3, offset=1)


@pytest.mark.parametrize("case", P.LAPLACE_PLAN_CASES, ids=lambda c: f"{_id(c)}-{c[2]}")
def test_every_plan_of_mode_apply(ctx, mem, case):
    res, bc, name = case
    ran = P.run_laplace_plans(ctx, mem, res, bc, _DT[name], batch=2, seed=4)
    assert ran == P.available_tiles(res[-1], _DT[name])


@DTYPES
@pytest.mark.parametrize("case", P.OBSTACLE_GRIDS, ids=_id)
def test_obstacle_kernels(ctx, mem, case, dtype):
    P.run_obstacles(ctx, mem, case[0], case[1], dtype, case[2], seed=5)


@pytest.mark.parametrize("case", P.ROW_CASES + SMALL, ids=_id)
def test_cell_flags_from_arbitrary_bytes(ctx, mem, case):
    rng = np.random.default_rng(6)
    for masks in (1, 3):
        for with_active in (True, False):
            pc.check_cellflags(ctx, mem, case[0], case[1], rng, batch_masks=masks, with_active=with_active)


# ---- the groups the emulation is too slow for ----------------------------------------------------------------------------------------------------------------------
def _device_group(fun):
    del P.RECORDS[:]
    try:
        fun()
    finally:
        P.report()


@DTYPES
@pytest.mark.parametrize("case", P.DEVICE_DIVERGENCE_CASES, ids=_id)
def test_divergence_with_several_planes_per_workgroup(ctx, mem, case, dtype):
    """ 2 planes per chunk, 2050 chunks, one plane in the last (asserted on the plan helper by the emulation file): lo0 = hi0, the clip of the last chunk, face0 at
    the wrap and at a CLOSED / OPEN pair with non-zero constants """
    res, bc, batch = case
    plan = P.divergence_plan(res, dtype)
    assert (plan["planes"], plan["chunks"], plan["last"]) == (2, 2050, 1)

    def run():
        for kind, mode in (("random", "none"), ("graded slow", "shared"), ("tiny", "none"), ("nonfinite", "shared")):
            P.check_divergence(ctx, mem, res, bc, dtype, batch, kind, mode, seed=7)
    _device_group(run)


@DTYPES
@pytest.mark.parametrize("case", P.DEVICE_GRAD_CASES, ids=_id)
def test_grad_subtract_second_trip_of_the_patch_loop(ctx, mem, case, dtype):
    res, bc, batch = case
    assert P.grad_subtract_plan(res, bc, dtype)["npatch"] > 16384

    def run():
        for kind, mode in (("random", "none"), ("graded slow", "shared")):
            P.check_grad_subtract(ctx, mem, res, bc, dtype, batch, kind, mode, seed=8)
    _device_group(run)


def test_balance_second_trip_of_the_grid_stride_loop(ctx, mem):
    res, bc, batch = P.DEVICE_BALANCE_CASE
    assert P.balance_plan(res)["trips"] == 2

    def run():
        for mode in ("none", "shared"):
            P.check_divergence(ctx, mem, res, bc, np.float32, batch, "random", mode, seed=9, variants=[(1, 0)])
    _device_group(run)

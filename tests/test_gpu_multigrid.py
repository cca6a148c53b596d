"""
`-m gpu`: Solve(..., preconditioner='multigrid') on the MI355X -- the cases of tests/test_multigrid_emu.py on the device, size independence of the iteration
count, the 384^3 fp64 cavity, and the captured step. Yardsticks as there (tests/multigrid_cases.py): the oracle's operator in float64 and the plain CG path.
Every case prints its figures before it asserts.
"""
import numpy as np
import pytest

import multigrid_cases as M
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


# ---- 9: tests 1, 2 and 4 on the device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(M.CASES))
def test_converges_and_needs_fewer_iterations(ctx, mem, name, dtype):
    M.check_converged_and_fewer(ctx, mem, name, dtype, 1e-5)


@pytest.mark.parametrize("name", list(M.CASES))
def test_converges_to_1e_10_in_fp64(ctx, mem, name):
    M.check_converged_and_fewer(ctx, mem, name, np.float64, 1e-10, compare=False)


def test_projection_with_an_obstacle(gpu_backend):
    M.check_projection(gpu_backend, 'A', np.float32)


def test_projection_with_a_batched_geometry(gpu_backend):
    M.check_projection(gpu_backend, 'D', np.float32, batched_geometry=True)


def test_projection_with_a_user_active_mask(gpu_backend):
    M.check_projection(gpu_backend, 'E', np.float32, user_active=True)


@pytest.mark.parametrize("name", ['A', 'C', 'D'])
def test_cycle_is_a_symmetric_operator_with_the_sign_of_A(ctx, mem, name):
    M.check_symmetric_operator(ctx, mem, name)


# ---- 10: size independence -----------------------------------------------------------------------------------------------------------------------------
def test_iterations_do_not_grow_with_the_resolution_3d(ctx, mem):
    """ closed box with a solid sphere, fp32, rel_tol 1e-5, 64^3 / 128^3 / 256^3; at 256^3 also <= plain CG's count / 10 """
    M.check_size_independence(ctx, mem, (64, 128, 256), 3, np.float32, 1e-5, plain_ratio=10)


def test_iterations_do_not_grow_with_the_resolution_2d(ctx, mem):
    """ closed box with a disc in fp64 (an fp32 residual of 1e-5 is at the edge of what a 2048^2 closed box allows), 256^2 / 1024^2 / 2048^2 """
    M.check_size_independence(ctx, mem, (256, 1024, 2048), 2, np.float64, 1e-5)


# ---- 11: 384^3 fp64 cavity with an obstacle at rel_tol 1e-10 -----------------------------------------------------------------------------------------
def test_cavity_384_fp64_to_1e_10(ctx, mem):
    case = M.closed_box_with_ball(ctx, mem, 384, 3, np.float64)
    rhs = case.noise(384)
    x, info = M.solve(ctx, mem, case, rhs, M.METHOD_MG, 1e-10)
    res = case.true_rel_residual(x, rhs)
    print(f"384^3 fp64 cavity: multigrid CG {info[0].iterations} iterations, true relative residual {res}, V-cycle {ctx.query_multigrid()}", flush=True)
    assert info[0].converged and not info[0].diverged
    assert float(res.max()) <= 2e-10
    x2, info2 = M.solve(ctx, mem, case, rhs, M.METHOD_MG, 1e-10)
    assert info2[0].iterations == info[0].iterations and np.array_equal(x, x2)


# ---- 12: the captured step ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dims", [(128, 'xy'), (64, 'xyz')])
def test_jit_compiled_step_replays_the_eager_bits(gpu_backend, n, dims):
    M.jit_step_matches_eager(gpu_backend, n, dims)


@pytest.mark.parametrize("name", ['A', 'D'])
def test_fixed_iterations_give_the_same_bits(ctx, mem, name):
    case = M.Case(ctx, mem, name, np.float32)
    rhs = case.noise(5).astype(np.float32)
    a, ia = M.solve(ctx, mem, case, rhs, M.METHOD_MG, 1e-5, max_iter=6, check=0)
    b, ib = M.solve(ctx, mem, case, rhs, M.METHOD_MG, 1e-5, max_iter=6, check=0)
    assert np.array_equal(a, b) and [i.iterations for i in ia] == [i.iterations for i in ib]

"""
Solve(..., preconditioner='multigrid') -- CG preconditioned by one geometric multigrid V-cycle per iteration (csrc/multigrid.hpp, phihip_method 2) -- on
the emulation library. Yardsticks: the oracle's operator in float64 and the library's own PLAIN CG path (tests/multigrid_cases.py), never the
multigrid path itself.
"""
import ctypes

import numpy as np
import pytest
import torch

import multigrid_cases as M
from parity_cases import CLO, OPN, C, NumpyMem, O, demean, rel_l2
from phiflow_amd import _capi
from phiflow_amd.flow import BOUNDARY, PERIODIC, ZERO, Box, CenteredGrid, NotConverged, Solve, StaggeredGrid, combine_sides, diffuse, fluid

MEM = NumpyMem()


# ---- 1 + 2: converged means converged; fewer iterations than plain CG on the same inputs ---------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(M.CASES))
def test_converges_and_needs_fewer_iterations(emu_ctx, name, dtype):
    M.check_converged_and_fewer(emu_ctx, MEM, name, dtype, 1e-5)


@pytest.mark.parametrize("name", list(M.CASES))
def test_converges_to_1e_10_in_fp64(emu_ctx, name):
    M.check_converged_and_fewer(emu_ctx, MEM, name, np.float64, 1e-10, compare=False)


def test_solve_linear_passes_the_preconditioner_on(emu_backend):
    """ the mirror's own solve_linear (phi/field/__init__.py:31) on case B's operator: converged, true residual by the oracle <= 4 rel_tol, fewer iterations """
    res, bc, _ = M.CASES['B']
    ext = combine_sides(x=BOUNDARY, y=(ZERO, BOUNDARY))
    bounds = Box['x,y', 0:res[0], 0:res[1]]
    rng = np.random.default_rng(3)
    rhs = rng.standard_normal(res).astype(np.float32)
    y = CenteredGrid(rhs, 0, bounds, x=res[0], y=res[1], backend=emu_backend)
    from phiflow_amd.linear import solve_linear
    x_mg = solve_linear(fluid.masked_laplace, y, Solve('CG', 1e-5, 0, preconditioner='multigrid'), ext)
    x_cg = solve_linear(fluid.masked_laplace, y, Solve('CG', 1e-5, 0, max_iterations=5000), ext)
    dom = O.Domain(res, (0.0, 0.0), tuple(float(r) for r in res), bc)
    r = rhs.astype(np.float64)[None] - O.masked_laplace(x_mg.numpy().astype(np.float64)[None], dom)
    assert x_mg.solve_info.converged == [True]
    assert np.sqrt((r ** 2).sum() / (rhs.astype(np.float64) ** 2).sum()) <= 4e-5
    assert x_mg.solve_info.iterations[0] <= x_cg.solve_info.iterations[0] / 4, (x_mg.solve_info.iterations, x_cg.solve_info.iterations)


# ---- 3: the cycle is a symmetric operator with the sign of A ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['A', 'C', 'D'])
def test_cycle_is_a_symmetric_operator_with_the_sign_of_A(emu_ctx, name):
    M.check_symmetric_operator(emu_ctx, MEM, name)


# ---- 4: the projection ---------------------------------------------------------------------------------------------------------------------------------
def test_projection_with_an_obstacle(emu_backend):
    M.check_projection(emu_backend, 'A', np.float32)


def test_projection_with_a_batched_geometry(emu_backend):
    M.check_projection(emu_backend, 'D', np.float32, batched_geometry=True)


def test_projection_with_a_user_active_mask(emu_backend):
    M.check_projection(emu_backend, 'E', np.float32, user_active=True)


# ---- 5: warm start and frozen entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_warm_start_and_frozen_entries(emu_ctx, dtype):
    tol = 1e-5
    single = M.Case(emu_ctx, MEM, 'A', dtype, 1)
    rhs = [single.noise(s).astype(dtype) for s in (21, 22, 23)]
    solo = [M.solve(emu_ctx, MEM, single, r, M.METHOD_MG, tol) for r in rhs]
    assert all(i[0].converged for _, i in solo)
    batch = M.Case(emu_ctx, MEM, 'A', dtype, 3)
    x0 = np.zeros((3,) + tuple(batch.dom.res), dtype)
    x0[0] = solo[0][0][0]                                # entry 0 starts from its converged pressure
    x, info = M.solve(emu_ctx, MEM, batch, np.concatenate(rhs), M.METHOD_MG, tol, x0=x0)
    assert all(i.converged for i in info)
    assert info[0].iterations in (0, 1), info[0].iterations
    assert rel_l2(x[0], x0[0]) <= 1e-6
    for b in (1, 2):
        assert abs(info[b].iterations - solo[b][1][0].iterations) <= 1, (b, info[b].iterations, solo[b][1][0].iterations)
        assert rel_l2(demean(x[b:b + 1]), demean(solo[b][0])) <= 1e-5


# ---- 6: fixed-iteration mode and the captured step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['A', 'D'])
def test_fixed_iterations_give_the_same_bits(emu_ctx, name):
    case = M.Case(emu_ctx, MEM, name, np.float32)
    rhs = case.noise(5).astype(np.float32)
    a, ia = M.solve(emu_ctx, MEM, case, rhs, M.METHOD_MG, 1e-5, max_iter=6, check=0)
    b, ib = M.solve(emu_ctx, MEM, case, rhs, M.METHOD_MG, 1e-5, max_iter=6, check=0)
    assert np.array_equal(a, b) and [i.iterations for i in ia] == [i.iterations for i in ib]
    assert all(i.iterations <= 6 for i in ia)


def test_jit_compiled_step_equals_the_eager_steps(emu_backend):
    M.jit_step_matches_eager(emu_backend, 24, 'xy')


# ---- 7: gradients ------------------------------------------------------------------------------------------------------------------------------------------
def _fd_gradient_check(loss_of_values, values, grads, rng, eps=1e-6, tol=2e-5, n_dirs=3):
    """ directional central differences of a scalar python function of a list of float64 arrays vs analytic gradients (as in tests/test_host_api.py) """
    for _ in range(n_dirs):
        d = [rng.standard_normal(v.shape) for v in values]
        plus = loss_of_values([v + eps * di for v, di in zip(values, d)])
        minus = loss_of_values([v - eps * di for v, di in zip(values, d)])
        fd = (plus - minus) / (2 * eps)
        an = float(sum(np.vdot(g, di) for g, di in zip(grads, d)))
        assert abs(fd - an) <= tol * max(abs(fd), abs(an), 1e-3), f"finite difference {fd} vs gradient {an}"


def test_make_incompressible_gradient_with_the_preconditioner(emu_backend):
    """ the form of test_make_incompressible_gradient (tests/test_host_api.py): fp64, 16 x 16, the three boundary mixes; the same finite-difference check
    with the same tol, and agreement with the gradient obtained without the preconditioner to 1e-8 relative """
    from phiflow_amd.flow import jacobian, l2_loss, precision
    rng = np.random.default_rng(20)
    with precision(64):
        bounds = Box['x,y', 0:100, 0:100]
        for ext in (ZERO, PERIODIC, combine_sides(x=BOUNDARY, y=(ZERO, BOUNDARY))):
            shapes = StaggeredGrid(0, ext, bounds, x=16, y=16, backend=emu_backend).component_shapes
            vals = [rng.standard_normal(s) for s in shapes]
            grads = {}
            for key, solve in (('mg', Solve('CG', 1e-12, 0, preconditioner='multigrid')), ('cg', Solve('CG', 1e-12, 0))):
                def sim(velocity):
                    velocity, _ = fluid.make_incompressible(velocity, (), solve)
                    loss = l2_loss(velocity)
                    assert bool(torch.isfinite(loss).all())
                    return loss
                grad, = jacobian(sim, get_output=False)(StaggeredGrid(vals, ext, bounds, x=16, y=16, backend=emu_backend))
                assert grad.is_staggered and all(np.isfinite(g).all() for g in grad.numpy())
                grads[key] = grad.numpy()
                if key == 'mg':
                    loss_np = lambda vs: float(sim(StaggeredGrid(vs, ext, bounds, x=16, y=16, backend=emu_backend)))
                    _fd_gradient_check(loss_np, vals, grad.numpy(), rng, tol=1e-6)
            a, b = np.concatenate([g.ravel() for g in grads['mg']]), np.concatenate([g.ravel() for g in grads['cg']])
            assert rel_l2(a, b) <= 1e-8, rel_l2(a, b)


# ---- 8: refusals and the unchanged default ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_unchanged_default(emu_backend, emu_library):
    with pytest.raises(NotImplementedError, match="CG-adaptive"):
        Solve('CG-adaptive', 1e-5, preconditioner='multigrid').to_c(False)
    with pytest.raises(NotImplementedError, match="multigrid"):
        Solve('CG', 1e-5, preconditioner='ilu').to_c(False)
    v = StaggeredGrid(0, 0, x=8, y=8, backend=emu_backend)
    with pytest.raises(NotImplementedError):
        fluid.make_incompressible(v, (), Solve('CG-adaptive', preconditioner='multigrid'))
    with pytest.raises(NotImplementedError):
        fluid.make_incompressible(v, (), Solve('CG', preconditioner='jacobi'))
    t = CenteredGrid(np.random.default_rng(0).standard_normal((8, 8)).astype(np.float32), 0, x=8, y=8, backend=emu_backend)
    with pytest.raises(NotImplementedError, match="preconditioner"):
        diffuse.implicit(t, 0.1, 1.0, Solve('CG', 1e-5, preconditioner='multigrid'))
    with pytest.raises(NotImplementedError, match="preconditioner"):
        diffuse.implicit(t, t * 0 + 0.1, 1.0, Solve('CG', 1e-5, preconditioner='multigrid'))
    from phiflow_amd.slab import SlabSolver
    import inspect
    assert 'preconditioner' in inspect.signature(SlabSolver.solve).parameters
    with pytest.raises(NotImplementedError, match="preconditioner"):
        SlabSolver.solve(None, None, None, preconditioner='multigrid')
    # the C layer refuses what it does not cover, too
    ctx = _capi.Context(emu_library, 0)
    grid = C.make_grid(2, C.PHIHIP_F32, 1, (8, 8), (0, 0), (8, 8), ((CLO, CLO), (OPN, OPN)))
    rhs, x = np.ones((1, 8, 8), np.float32), np.zeros((1, 8, 8), np.float32)
    mg = _capi.Solve(1e-5, 0.0, 100, 50, 10, 2)
    with pytest.raises(_capi.PhiHipError) as e:
        ctx.cg_solve_shifted(grid, 1.0, -0.1, rhs.ctypes.data, x.ctypes.data, mg)
    assert e.value.status == -3
    with pytest.raises(_capi.PhiHipError):
        ctx.cg_solve(grid, 0, 1, rhs.ctypes.data, x.ctypes.data, _capi.Solve(1e-5, 0.0, 100, 50, 10, 3))
    # the default is what it was
    s = Solve('CG', 1e-3, 1e-4, None, 500, (NotConverged,))
    assert (s.method, s.rel_tol, s.abs_tol, s.x0, s.max_iterations, s.suppress, s.preconditioner) == ('CG', 1e-3, 1e-4, None, 500, (NotConverged,), None)
    assert Solve().to_c(False).method == 0 and Solve('CG-adaptive').to_c(False).method == 1
    assert Solve('auto', preconditioner='multigrid').to_c(False).method == 2 and Solve('CG', preconditioner='multigrid').to_c(True).method == 2
    assert ctypes.sizeof(_capi.Solve) == 32
    # the workspace grows with the first preconditioned solve and the context destroys cleanly
    before = ctx.workspace_bytes()
    ctx.cg_solve(grid, 0, 1, rhs.ctypes.data, x.ctypes.data, mg)
    assert ctx.workspace_bytes() > before
    q = ctx.query_multigrid()
    assert q["levels"] == 2 and q["launches"] > 0
    del ctx

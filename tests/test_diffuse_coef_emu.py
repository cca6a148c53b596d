"""
diffuse.explicit / diffuse.implicit with a spatially varying and per-axis diffusivity (phi/physics/diffuse.py:13-60, :98-141; Heat_Flow.ipynb) on the
emulation library, against the fp64 NumPy restatement of tests/diffuse_coef_ref.py (flux form on all n + 1 faces, min of the signed amounts).
"""
import warnings

import numpy as np
import pytest
import torch

from phiflow_amd.flow import (PERIODIC, ZERO_GRADIENT, Box, CenteredGrid, NotConverged, Solve, StaggeredGrid, combine_sides, diffuse, precision,
                              union, vec)
from phiflow_amd.diffuse import _scalar_walls

import diffuse_coef_ref as R


def _walls(f):
    codes, vals = _scalar_walls(f)
    return [list(c) for c in codes], vals


def _rng_field(rng, shape, batch, boundary, backend, lo=0.0, hi=1.0, **res):
    arr = rng.uniform(lo, hi, (batch,) + shape) if batch else rng.uniform(lo, hi, shape)
    return CenteredGrid(arr, boundary, backend=backend, **res), arr


U_WALLS = {
    'periodic': PERIODIC,
    'zero_gradient': ZERO_GRADIENT,
    'constant': 0.7,
    'mixed': combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC, z=(ZERO_GRADIENT, -0.5)),
}
A_WALLS = {'zero': 0.0, 'zero_gradient': ZERO_GRADIENT, 'periodic': PERIODIC, 'constant': 2.5}


def _mixed2(ext):
    """ the 3-D mixed extrapolation restricted to x, y """
    return combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC) if ext is U_WALLS['mixed'] else ext


def test_explicit_centered_non_isotropic(emu_backend):
    """ tests/commit/physics/test_diffuse.py:69-80: a scalar, vec(x=1, y=2) and CenteredGrid(1, x=4, y=4) * (1, 2) """
    grid = CenteredGrid(np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32), 0, x=3, y=3, backend=emu_backend)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # (CFL 1 > 0.5, as in the reference)
        iso = diffuse.explicit(grid, 1, 1).numpy()
        np.testing.assert_array_equal(iso, [[0, 1, 0], [1, -3, 1], [0, 1, 0]])
        expected = [[0, 1, 0], [2, -5, 2], [0, 1, 0]]
        np.testing.assert_array_equal(diffuse.explicit(grid, vec(x=1, y=2), 1).numpy(), expected)
        np.testing.assert_array_equal(diffuse.explicit(grid, (1, 2), 1).numpy(), expected)
        field = CenteredGrid(1, x=4, y=4, backend=emu_backend) * (1, 2)
        np.testing.assert_array_equal(diffuse.explicit(grid, field, 1).numpy(), expected)
        # an isotropic vector is the number: the same kernels, the same bits
        np.testing.assert_array_equal(diffuse.explicit(grid, vec(x=1, y=1), 1).numpy(), iso)


@pytest.mark.parametrize("uw", list(U_WALLS))
@pytest.mark.parametrize("aw", list(A_WALLS))
def test_explicit_field_against_restatement(emu_backend, uw, aw):
    rng = np.random.default_rng(hash((uw, aw)) % 2 ** 32)
    # 2-D fp32, batch 2 with a shared diffusivity, substeps 3
    ub, ab = _mixed2(U_WALLS[uw]), A_WALLS[aw]
    bounds = Box['x,y', 0:3, 0:2]
    u, u_np = _rng_field(rng, (12, 10), 2, ub, emu_backend, -1, 1, x=12, y=10, bounds=bounds)
    a, a_np = _rng_field(rng, (12, 10), 0, ab, emu_backend, 0.1, 1.0, x=12, y=10, bounds=bounds)
    out = diffuse.explicit(u, a * (1.0, 0.5), 0.01, substeps=3).numpy()
    uc, uv = _walls(u)
    ac, av = _walls(a)
    ref = R.explicit(u_np.astype(np.float32), a_np.astype(np.float32)[None], [0.01, 0.005], u.dx, uc, uv, ac, av, substeps=3)
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)
    # 3-D fp64, batch 2 with a diffusivity per batch entry
    with precision(64):
        bounds3 = Box['x,y,z', 0:1, 0:1.5, 0:1]
        u, u_np = _rng_field(rng, (6, 5, 7), 2, U_WALLS[uw], emu_backend, -1, 1, x=6, y=5, z=7, bounds=bounds3)
        a, a_np = _rng_field(rng, (6, 5, 7), 2, ab, emu_backend, 0.1, 1.0, x=6, y=5, z=7, bounds=bounds3)
        out = diffuse.explicit(u, a, 0.002).numpy()
        uc, uv = _walls(u)
        ac, av = _walls(a)
        ref = R.explicit(u_np, a_np, [0.002] * 3, u.dx, uc, uv, ac, av)
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-13)


def test_explicit_resampled_and_constant_field(emu_backend):
    rng = np.random.default_rng(5)
    u, u_np = _rng_field(rng, (16, 8), 0, ZERO_GRADIENT, emu_backend, 0, 1, x=16, y=8, bounds=Box['x,y', 0:4, 0:2])
    # a diffusivity on a coarser grid of the same box: `amount.at(u)` = the grid-to-grid sampling, keeping its own extrapolation
    coarse = CenteredGrid(rng.uniform(0.1, 1, (8, 4)), ZERO_GRADIENT, x=8, y=4, bounds=Box['x,y', 0:4, 0:2], backend=emu_backend)
    onu = (coarse @ u)
    out = diffuse.explicit(u, coarse, 0.01).numpy()
    np.testing.assert_array_equal(out, diffuse.explicit(u, CenteredGrid(onu.values, ZERO_GRADIENT, x=16, y=8, bounds=Box['x,y', 0:4, 0:2],
                                                                        backend=emu_backend), 0.01).numpy())
    uc, uv = _walls(u)
    ref = R.explicit(u_np[None].astype(np.float32), onu.numpy()[None], [0.01, 0.01], u.dx, uc, uv, [[R.OPEN] * 2] * 2, [[0, 0]] * 2)
    np.testing.assert_allclose(out, ref[0], rtol=1e-5, atol=1e-6)
    # a constant field (zero-gradient: no wall effect) equals the float path to rounding
    const = CenteredGrid(0.3, ZERO_GRADIENT, x=16, y=8, bounds=Box['x,y', 0:4, 0:2], backend=emu_backend)
    np.testing.assert_allclose(diffuse.explicit(u, const, 0.05).numpy(), diffuse.explicit(u, 0.3, 0.05).numpy(), rtol=1e-6, atol=1e-7)


def test_signed_minimum_two_cells(emu_backend):
    """ 2 cells along x, a = (1, 3) with a ZERO extrapolation, u walls constant 2: dt > 0 takes the min (and the walls insulate: min(w a, 0) = 0),
    dt < 0 (implicit's sharpen) the max (and the walls conduct: min(-|w| a, 0) = -|w| a) -- computed by hand """
    with precision(64):
        u = CenteredGrid(np.array([[1.0], [0.0]]), combine_sides(x=2.0, y=ZERO_GRADIENT), x=2, y=1, bounds=Box['x,y', 0:2, 0:1], backend=emu_backend)
        a = CenteredGrid(np.array([[1.0], [3.0]]), 0.0, x=2, y=1, bounds=Box['x,y', 0:2, 0:1], backend=emu_backend)
        fwd = diffuse.explicit(u, a, 0.1).numpy()[:, 0]
        # face 1/2: min(.1, .3) = .1 ; walls: min(.1, 0) = min(.3, 0) = 0
        np.testing.assert_allclose(fwd, [1 + 0.1 * (0 - 1), 0 - 0.1 * (0 - 1)], rtol=1e-14)
        bwd = diffuse.explicit(u, a, -0.1).numpy()[:, 0]
        # face 1/2: min(-.1, -.3) = -.3 ; lower wall min(-.1, 0) = -.1 ; upper wall min(-.3, 0) = -.3
        F_lo, F_mid, F_hi = -0.1 * (1 - 2), -0.3 * (0 - 1), -0.3 * (2 - 0)
        np.testing.assert_allclose(bwd, [1 + F_mid - F_lo, 0 + F_hi - F_mid], rtol=1e-14)


def _heat_flow(backend, nx=20, ny=10):
    domain = Box(x=10, y=5)
    bars = union(Box(x=(0, 10), y=(2, 3)), Box(x=(4.5, 5.5), y=(1, 4)))
    conductivity = CenteredGrid(bars, ZERO_GRADIENT, domain, x=nx, y=ny, backend=backend) + .01
    t0 = CenteredGrid(0, {'x-': 1, 'x+': ZERO_GRADIENT, 'y': PERIODIC}, domain, x=nx, y=ny, backend=backend)
    return conductivity, t0


def test_implicit_heat_flow_against_direct_solve(emu_backend):
    conductivity, t = _heat_flow(emu_backend)
    tc, tv = _walls(t)
    ac, av = _walls(conductivity)
    a_np = conductivity.numpy()[None]
    ref = t.numpy()[None].astype(np.float64)
    for _ in range(5):
        t = diffuse.implicit(t, conductivity, 1.0, Solve('CG', 1e-6, 0))
        assert t.solve_info.converged == [True]
        ref = R.implicit(ref, a_np, [1.0, 1.0], t.dx, tc, tv, ac, av)
        np.testing.assert_allclose(t.numpy(), ref[0], atol=2e-5)
    vals = t.numpy()
    assert vals.min() >= 0 and vals.max() <= 1 + 1e-5 and vals[0].min() > 0.1     # heat enters through the x- wall only
    assert vals[-1, 4:6].min() > 10 * vals[-1].max(where=np.abs(np.arange(10) - 4.5) > 2, initial=0)   # ... and travels along the bar


@pytest.mark.parametrize("method", ['CG', 'CG-adaptive'])
def test_implicit_random_field(emu_backend, method):
    rng = np.random.default_rng(11)
    with precision(64):
        for ub, ab in ((0.7, PERIODIC), (combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC, z=ZERO_GRADIENT), 0.0)):
            u, u_np = _rng_field(rng, (6, 5, 7), 2, ub, emu_backend, -1, 1, x=6, y=5, z=7)
            a, a_np = _rng_field(rng, (6, 5, 7), 1, ab, emu_backend, 0.1, 2.0, x=6, y=5, z=7)
            out = diffuse.implicit(u, a * (1, 2, 0.5), 0.3, Solve(method, 1e-10, 0, max_iterations=500))
            uc, uv = _walls(u)
            ac, av = _walls(a)
            kdt = [0.3, 0.6, 0.15]
            res = R.implicit_residual(out.numpy(), u_np, a_np, kdt, u.dx, uc, uv, ac, av)
            assert res.max() <= 1e-10, res
            np.testing.assert_allclose(out.numpy(), R.implicit(u_np, a_np, kdt, u.dx, uc, uv, ac, av), atol=1e-9)
    # per-axis constants without a field, fp32
    u, u_np = _rng_field(rng, (12, 10), 0, ZERO_GRADIENT, emu_backend, 0, 1, x=12, y=10)
    out = diffuse.implicit(u, vec(x=0.5, y=2.0), 1.0, Solve(method, 1e-6, 0))
    uc, uv = _walls(u)
    res = R.implicit_residual(out.numpy()[None], u_np[None], None, [0.5, 2.0], u.dx, uc, uv)
    assert res.max() <= 1e-6 * 1.5, res


def test_implicit_conservation_bounds_and_failure(emu_backend):
    rng = np.random.default_rng(2)
    step = np.zeros((16, 12)); step[:8] = 1
    a, _ = _rng_field(rng, (16, 12), 0, ZERO_GRADIENT, emu_backend, 0.05, 3.0, x=16, y=12)
    with precision(64):
        a64 = CenteredGrid(a.numpy().astype(np.float64), ZERO_GRADIENT, x=16, y=12, backend=emu_backend)
        for ext in (PERIODIC, ZERO_GRADIENT):
            u = CenteredGrid(step, ext, x=16, y=12, backend=emu_backend)
            out = diffuse.implicit(u, a64, 2.0, Solve('CG', 1e-12, 0, max_iterations=2000)).numpy()
            assert abs(out.sum() - step.sum()) <= 1e-8 * step.sum()
            assert out.min() >= -1e-10 and out.max() <= 1 + 1e-10
            ex = diffuse.explicit(u, a64, 0.02).numpy()          # (the explicit flux form conserves too)
            assert abs(ex.sum() - step.sum()) <= 1e-10 * step.sum()
    u = CenteredGrid(step, ZERO_GRADIENT, x=16, y=12, backend=emu_backend)
    with pytest.raises(NotConverged):
        diffuse.implicit(u, a, 50.0, Solve('CG', 1e-7, 0, max_iterations=2))
    out = diffuse.implicit(u, a, 50.0, Solve('CG', 1e-7, 0, max_iterations=2, suppress=[NotConverged]))
    assert out.solve_info.iterations == [2]


def test_adjoint_identity(emu_backend):
    """ <L g, h> = <g, L h> with the vector-Jacobian products of torch.autograd (homogeneous walls: the operator is linear and symmetric) """
    rng = np.random.default_rng(8)
    with precision(64):
        ext = combine_sides(x=(0.0, ZERO_GRADIENT), y=PERIODIC)
        a, _ = _rng_field(rng, (10, 8), 0, 0.5, emu_backend, 0.1, 1, x=10, y=8)
        g = torch.tensor(rng.standard_normal((1, 10, 8)), requires_grad=True)
        h = torch.tensor(rng.standard_normal((1, 10, 8)))
        for op in (lambda f: diffuse.explicit(f, a * (1, 3), 0.01, substeps=2), lambda f: diffuse.implicit(f, a * (1, 3), 0.5, Solve('CG', 1e-12, 0))):
            Lg = op(CenteredGrid(g, ext, x=10, y=8, backend=emu_backend)).values
            (vjp,) = torch.autograd.grad((Lg * h).sum(), g)          # = L^T h
            Lh = op(CenteredGrid(h, ext, x=10, y=8, backend=emu_backend)).values
            lhs, rhs = float((Lg.detach() * h).sum()), float((g.detach() * Lh).sum())
            assert abs(lhs - rhs) <= 1e-9 * abs(lhs)
            np.testing.assert_allclose(vjp.numpy(), Lh.numpy(), rtol=1e-9, atol=1e-11)


def test_refused_forms(emu_backend):
    v = StaggeredGrid(0, 0, x=8, y=8, backend=emu_backend)
    a = CenteredGrid(1, x=8, y=8, backend=emu_backend)
    with pytest.raises(NotImplementedError, match="centred"):
        diffuse.explicit(v, a, 0.1)
    with pytest.raises(NotImplementedError, match="centred"):
        diffuse.implicit(v, a, 0.1)
    with pytest.raises(NotImplementedError):
        diffuse.explicit(v, vec(x=1, y=2), 0.1)
    u = CenteredGrid(0, ZERO_GRADIENT, x=8, y=8, backend=emu_backend)
    ag = CenteredGrid(torch.ones(1, 8, 8, requires_grad=True), x=8, y=8, backend=emu_backend)
    with pytest.raises(NotImplementedError, match="diffusivity"):
        diffuse.explicit(u, ag, 0.1)
    with pytest.raises(NotImplementedError, match="diffusivity"):
        diffuse.implicit(u, ag, 0.1)

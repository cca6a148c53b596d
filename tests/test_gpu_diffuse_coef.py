"""
diffuse.explicit / diffuse.implicit with a spatially varying and per-axis diffusivity on the MI355X (csrc/diffuse_coef.hpp), against the fp64
NumPy restatement of tests/diffuse_coef_ref.py; implicit solves are judged by their true residual under the restated operator.
"""
import numpy as np
import pytest
import torch

from phiflow_amd.flow import (PERIODIC, ZERO_GRADIENT, Box, CenteredGrid, Solve, combine_sides, diffuse, jit_compile, precision, union)
from phiflow_amd.diffuse import _scalar_walls

import diffuse_coef_ref as R

pytestmark = pytest.mark.gpu


def _walls(f):
    codes, vals = _scalar_walls(f)
    return [list(c) for c in codes], vals


CASES_2D = [(PERIODIC, ZERO_GRADIENT), (ZERO_GRADIENT, 0.0), (0.7, PERIODIC), (combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC), 2.5)]
CASES_3D = [(PERIODIC, PERIODIC), (combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC, z=(ZERO_GRADIENT, -0.5)), 0.0), (0.7, ZERO_GRADIENT)]


@pytest.mark.parametrize("case", range(len(CASES_2D)))
def test_explicit_and_implicit_2d_batch(gpu_backend, case):
    ub, ab = CASES_2D[case]
    rng = np.random.default_rng(case)
    u_np = rng.uniform(-1, 1, (4, 128, 128))
    for a_batch in (1, 4):
        a_np = rng.uniform(0.1, 1.0, (a_batch, 128, 128))
        u = CenteredGrid(u_np, ub, Box['x,y', 0:2, 0:1], x=128, y=128, backend=gpu_backend)
        a = CenteredGrid(a_np, ab, Box['x,y', 0:2, 0:1], x=128, y=128, backend=gpu_backend)
        uc, uv = _walls(u)
        ac, av = _walls(a)
        out = diffuse.explicit(u, a * (1.0, 0.5), 1e-5, substeps=3).numpy()
        ref = R.explicit(u_np.astype(np.float32), a_np.astype(np.float32), [1e-5, 0.5e-5], u.dx, uc, uv, ac, av, substeps=3)
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)
        sol = diffuse.implicit(u, a * (1.0, 0.5), 1e-3, Solve('CG', 1e-5, 0, max_iterations=2000))
        assert all(sol.solve_info.converged)
        res = R.implicit_residual(sol.numpy(), u.numpy(), a_np.astype(np.float32), [1e-3, 0.5e-3], u.dx, uc, uv, ac, av)
        assert res.max() <= 2e-5, res


@pytest.mark.parametrize("case", range(len(CASES_3D)))
@pytest.mark.parametrize("bits", [32, 64])
def test_explicit_and_implicit_3d(gpu_backend, case, bits):
    ub, ab = CASES_3D[case]
    rng = np.random.default_rng(10 + case)
    n = 64
    with precision(bits):
        u_np = rng.uniform(-1, 1, (n, n, n))
        a_np = rng.uniform(0.1, 1.0, (n, n, n))
        u = CenteredGrid(u_np, ub, x=n, y=n, z=n, backend=gpu_backend)
        a = CenteredGrid(a_np, ab, x=n, y=n, z=n, backend=gpu_backend)
        uc, uv = _walls(u)
        ac, av = _walls(a)
        cast = np.float32 if bits == 32 else np.float64
        out = diffuse.explicit(u, a, 0.1).numpy()
        ref = R.explicit(u_np.astype(cast)[None], a_np.astype(cast)[None], [0.1] * 3, u.dx, uc, uv, ac, av)[0]
        np.testing.assert_allclose(out, ref, rtol=1e-5 if bits == 32 else 1e-12, atol=1e-6 if bits == 32 else 1e-13)
        rtol = 1e-5 if bits == 32 else 1e-10
        for method in ('CG', 'CG-adaptive'):
            sol = diffuse.implicit(u, a * (1, 2, 0.5), 1.0, Solve(method, rtol, 0, max_iterations=3000))
            assert all(sol.solve_info.converged)
            res = R.implicit_residual(sol.numpy()[None], u.numpy()[None], a_np.astype(cast)[None], [1.0, 2.0, 0.5], u.dx, uc, uv, ac, av)
            assert res.max() <= 2 * rtol, res


def test_explicit_256_and_determinism(gpu_backend):
    rng = np.random.default_rng(3)
    n = 256
    u_np = rng.uniform(-1, 1, (n, n, n)).astype(np.float32)
    a_np = rng.uniform(0.1, 1.0, (n, n, n)).astype(np.float32)
    ub = combine_sides(x=(1.0, ZERO_GRADIENT), y=PERIODIC, z=0.0)
    u = CenteredGrid(u_np, ub, x=n, y=n, z=n, backend=gpu_backend)
    a = CenteredGrid(a_np, ZERO_GRADIENT, x=n, y=n, z=n, backend=gpu_backend)
    out = diffuse.explicit(u, a, 0.1)
    uc, uv = _walls(u)
    ac, av = _walls(a)
    ref = R.explicit(u_np[None], a_np[None], [0.1] * 3, u.dx, uc, uv, ac, av)[0]
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5, atol=1e-6)
    assert torch.equal(out.values, diffuse.explicit(u, a, 0.1).values)
    s1 = diffuse.implicit(u, a, 1.0, Solve('CG', 1e-5, 0, max_iterations=500))
    s2 = diffuse.implicit(u, a, 1.0, Solve('CG', 1e-5, 0, max_iterations=500))
    assert torch.equal(s1.values, s2.values) and s1.solve_info.iterations == s2.solve_info.iterations


def _heat_flow(backend, nx=100, ny=50):
    domain = Box(x=10, y=5)
    bars = union(Box(x=(0, 10), y=(2, 3)), Box(x=(4.5, 5.5), y=(1, 4)))
    conductivity = CenteredGrid(bars, ZERO_GRADIENT, domain, x=nx, y=ny, backend=backend) + .01
    t0 = CenteredGrid(0, {'x-': 1, 'x+': ZERO_GRADIENT, 'y': PERIODIC}, domain, x=nx, y=ny, backend=backend)
    return conductivity, t0


def test_heat_flow_direct_solve_and_jit_replay(gpu_backend):
    conductivity, t = _heat_flow(gpu_backend, 20, 10)
    tc, tv = _walls(t)
    ac, av = _walls(conductivity)
    ref = t.numpy()[None].astype(np.float64)
    for _ in range(5):
        t = diffuse.implicit(t, conductivity, 1.0, Solve('CG', 1e-6, 0))
        ref = R.implicit(ref, conductivity.numpy()[None], [1.0, 1.0], t.dx, tc, tv, ac, av)
        np.testing.assert_allclose(t.numpy(), ref[0], atol=2e-5)
    # the notebook's jit_compile'd step, replayed 10 times, equals the eager steps bit for bit
    conductivity, t0 = _heat_flow(gpu_backend)

    def step(t, dt):
        return diffuse.implicit(t, conductivity, dt)
    jstep = jit_compile(step)
    eager, traced = t0, t0
    for _ in range(10):
        eager = step(eager, 1.0)
        traced = jstep(traced, 1.0)
        assert torch.equal(eager.values, traced.values)
    assert float(traced.values.max()) > 0.5

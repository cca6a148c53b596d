"""
Centred vector fields on the MI355X (csrc/advect_cvec.hpp): the fused advection by a centred velocity against the fp64 restatement of
tests/centered_vector_ref.py at 256^2 x 8 and 96^3, an exact whole-cell translation at 256^3, staggered <-> centres against the oracle and the
jit_compile'd Burgers step against the eager one.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from phiflow_amd.flow import PERIODIC, ZERO_GRADIENT, Box, CenteredGrid, StaggeredGrid, advect, combine_sides, jit_compile, precision
from phiflow_amd.field import _centered_rule

import centered_vector_ref as R
from centered_vector_ref import O
from parity_cases import advect_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cvec(arr, ext, bounds, backend):
    res = dict(zip('xyz', arr.shape[2:]))
    a = np.moveaxis(arr, 1, -1)
    return CenteredGrid(a if arr.shape[0] > 1 else a[0], ext, bounds, backend=backend, **res)


def _rule(f):
    codes, consts = _centered_rule(f, 'test')
    return [list(c) for c in codes], consts


CASES = {
    2: [(256, 256), Box(x=(0, 256), y=(0, 128)), [PERIODIC, combine_sides(x=(0.7, ZERO_GRADIENT), y=PERIODIC)], 8],
    3: [(96, 96, 96), Box(x=(0, 96), y=(0, 48), z=(0, 96)), [ZERO_GRADIENT, combine_sides(x=PERIODIC, y=(0.5, ZERO_GRADIENT), z=0.0)], 1],
}


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", [0, 1])
def test_fused_advection_parity(gpu_backend, D, bits, case):
    shape, bounds, exts, B = CASES[D]
    ext = exts[case]
    dtype = np.float32 if bits == 32 else np.float64
    rng = np.random.default_rng(10 * D + case)
    dx = [(u - l) / n for l, u, n in zip(bounds.lower, bounds.upper, shape)]
    dom = R._dom(shape, bounds.lower, bounds.upper)
    with precision(bits):
        vel_arr = rng.uniform(-1, 1, (B, D) + shape).astype(dtype)
        vel = _cvec(vel_arr, ext, bounds, gpu_backend)
        codes, consts = _rule(vel)
        amp = max(1.0, max(abs(c) for pair in consts for c in pair))
        for disp in (0.3, 2.7):
            dt = disp * min(dx)
            out = advect.semi_lagrangian(vel, vel, dt)                       # self-advection
            ref = R.semi_lagrangian(vel_arr, vel_arr, dt, shape, bounds.lower, bounds.upper, codes, consts)
            assert np.abs(out.numpy().reshape(ref.shape[0], *shape, D) - np.moveaxis(ref, 1, -1)).max() / amp <= advect_tol(dtype, dom)
        f_arr = rng.uniform(-1, 1, (B, D) + shape).astype(dtype)
        s_arr = rng.uniform(-1, 1, (B,) + shape).astype(dtype)
        v1 = vel_arr[:1]
        v1f = _cvec(v1, ext, bounds, gpu_backend)
        field = _cvec(f_arr, ext, bounds, gpu_backend)
        scalar = CenteredGrid(s_arr if B > 1 else s_arr[0], ext, bounds, backend=gpu_backend, **dict(zip('xyz', shape)))
        dt = 1.3 * min(dx)
        got = advect.semi_lagrangian(field, v1f, dt).values.cpu().numpy()
        ref = R.semi_lagrangian(f_arr, v1, dt, shape, bounds.lower, bounds.upper, codes, consts)
        assert np.abs(got - ref).max() / amp <= advect_tol(dtype, dom)
        got = advect.semi_lagrangian(scalar, v1f, dt).values.cpu().numpy()
        ref = R.semi_lagrangian(s_arr[:, None], v1, dt, shape, bounds.lower, bounds.upper, codes, consts)[:, 0]
        assert np.abs(got - ref).max() / amp <= advect_tol(dtype, dom)


def test_exact_translation_256(gpu_backend):
    """ a uniform velocity of whole cells (2, -1, 3) with unit cells on a periodic grid: the advection is a roll, bit for bit """
    n = 256
    with precision(32):
        torch.manual_seed(0)
        f = torch.randn((1, 3, n, n, n), dtype=torch.float32, device=gpu_backend.device)
        field = CenteredGrid(torch.movedim(f[0], 0, -1), PERIODIC, x=n, y=n, z=n, backend=gpu_backend)
        vel = CenteredGrid((2.0, -1.0, 3.0), PERIODIC, x=n, y=n, z=n, backend=gpu_backend)
        out = advect.semi_lagrangian(field, vel, 1.0).values
        assert torch.equal(out, torch.roll(f, shifts=(2, -1, 3), dims=(2, 3, 4)))
        s = field['y']
        assert torch.equal(advect.semi_lagrangian(s, vel, 1.0).values, torch.roll(s.values, shifts=(2, -1, 3), dims=(1, 2, 3)))
        del f, field, out


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("box", ['periodic', 'closed', 'open'])
def test_staggered_centres_round_trip_against_oracle(gpu_backend, D, box):
    shape = (64, 48) if D == 2 else (32, 24, 16)
    bounds = Box(**{d: (0.0, float(s) * (a + 1) / 2) for a, (d, s) in enumerate(zip('xyz', shape))})
    code = {'periodic': O.PERIODIC, 'closed': O.CLOSED, 'open': O.OPEN}[box]
    dom = O.Domain(shape, bounds.lower, bounds.upper, [(code, code)] * D)
    rng = np.random.default_rng(D)
    with precision(64):
        boundary = {'periodic': PERIODIC, 'closed': 0.0, 'open': ZERO_GRADIENT}[box]
        v = StaggeredGrid(0, boundary, bounds, backend=gpu_backend, **dict(zip('xyz', shape)))
        comps = [rng.uniform(-1, 1, tuple(c.shape[1:])) for c in v.values]
        v = v.with_values([torch.as_tensor(c[None], device=gpu_backend.device) for c in comps])
        c = v.at_centers()
        ref = np.stack(O.staggered_at_centers([a[None] for a in comps], dom), axis=1)
        np.testing.assert_allclose(c.values.cpu().numpy(), ref, rtol=0, atol=1e-14)
        ext = PERIODIC if box == 'periodic' else 0.4
        cv = c.with_boundary(ext)
        faces = StaggeredGrid(cv, boundary, bounds, backend=gpu_backend, **dict(zip('xyz', shape)))
        codes, consts = _rule(cv)
        for d in range(D):
            r = O.centered_to_staggered(np.ascontiguousarray(ref[:, d]), dom, codes, consts)[d]
            np.testing.assert_allclose(faces.values[d].cpu().numpy(), r, rtol=0, atol=1e-14)


def test_jit_burgers_step_bits_256(gpu_backend):
    spec = importlib.util.spec_from_file_location("burgers_example", os.path.join(ROOT, "examples", "burgers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    v0 = mod.initial_velocity(256, backend=gpu_backend)
    eager = v0
    for _ in range(3):
        eager = mod.step(eager)
    jitted = jit_compile(mod.step)
    out = v0
    for _ in range(3):
        out = jitted(out)
    assert out.is_vector
    np.testing.assert_array_equal(out.numpy(), eager.numpy())

"""
Grid differential operators (phiflow_amd.field: laplace, spatial_gradient(at='center'), divergence of a centred vector field, curl; csrc/diffops.hpp)
on the emulation library: element-wise forward and backward parity against the float64 restatements of tests/diffops_ref.py, layout and
metadata, hand values, jit_compile, the two example steps (examples/reaction_diffusion.py, examples/waves.py) and the refusals.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from phiflow_amd import field
from phiflow_amd.flow import (BOUNDARY, PERIODIC, ZERO, ZERO_GRADIENT, Box, CenteredGrid, Sphere, StaggeredGrid, combine_sides, curl, jit_compile, laplace,
                              precision, vec, where)

import diffops_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(name):
    spec = importlib.util.spec_from_file_location(f"{name}_example", os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. forward, element by element -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_laplace_centred(emu_backend, shape, name):
    C.check_laplace_centred(emu_backend, shape, name)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_laplace_staggered(emu_backend, shape, name):
    C.check_laplace_staggered(emu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_gradient_centred(emu_backend, shape, name):
    C.check_gradient(emu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_divergence_centred(emu_backend, shape, name):
    C.check_divergence(emu_backend, shape, name)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_curl_staggered(emu_backend, shape, name):
    C.check_curl_staggered(emu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_curl_centred(emu_backend, shape, name):
    C.check_curl_centred(emu_backend, shape, name)


# ---- 2. layout and metadata -------------------------------------------------------------------------------------------------------------------
def test_result_kinds_and_extrapolations(emu_backend):
    b = Box(x=(0.3, 2.1), y=(-1.0, 1.5))
    mixed = combine_sides(x=PERIODIC, y=(0.7, ZERO_GRADIENT))
    for ext, lap, div in ((PERIODIC, PERIODIC, PERIODIC), (ZERO_GRADIENT, ZERO, ZERO_GRADIENT), (0.7, ZERO, ZERO),
                          (mixed, combine_sides(x=PERIODIC, y=(ZERO, ZERO)), combine_sides(x=PERIODIC, y=(ZERO, ZERO_GRADIENT)))):
        s = CenteredGrid(1.0, ext, b, x=5, y=7, backend=emu_backend)
        v = CenteredGrid((1.0, 2.0), ext, b, x=5, y=7, backend=emu_backend)
        out = laplace(s)
        assert out.is_centered and not out.is_vector and out.boundary == lap and out.bounds is s.bounds and out.shape == s.shape
        assert v.laplace().is_vector and v.laplace().boundary == lap
        g = field.spatial_gradient(s, at='center')
        assert g.is_vector and tuple(g.values.shape) == (1, 2, 5, 7) and g.boundary == s.boundary.spatial_gradient()
        assert field.spatial_gradient(s, boundary=ZERO_GRADIENT, at='center').boundary == ZERO_GRADIENT
        d = field.divergence(v)
        assert d.is_centered and not d.is_vector and d.boundary == div and d.shape == s.shape
        for vel in (v, StaggeredGrid(0.5, ext, b, x=5, y=7, backend=emu_backend)):
            c = curl(vel)
            assert c.is_centered and not c.is_vector and c.resolution == {'x': 6, 'y': 8} and c.boundary == vel.boundary.spatial_gradient()
            dx, dy = vel.dx
            np.testing.assert_allclose(c.bounds.lower, (0.3 - dx / 2, -1.0 - dy / 2), rtol=0, atol=1e-15)
            np.testing.assert_allclose(c.bounds.upper, (2.1 + dx / 2, 1.5 + dy / 2), rtol=0, atol=1e-15)
            np.testing.assert_allclose(c.dx, vel.dx, rtol=1e-14)
    # the default location of the mirror stays 'face'
    assert field.spatial_gradient(CenteredGrid(1.0, ZERO_GRADIENT, b, x=5, y=7, backend=emu_backend)).is_staggered


def test_staggered_laplace_of_boundary_has_the_face_layout_of_zero(emu_backend):
    v = StaggeredGrid(0.5, BOUNDARY, x=5, y=7, backend=emu_backend)
    out = v.laplace()
    assert out.is_staggered and out.boundary == ZERO
    assert [tuple(t.shape[1:]) for t in out.values] == StaggeredGrid(0, ZERO, x=5, y=7, backend=emu_backend).component_shapes == [(4, 7), (5, 6)]
    per = StaggeredGrid(0.5, PERIODIC, x=5, y=7, backend=emu_backend).laplace()
    assert per.boundary == PERIODIC and [tuple(t.shape[1:]) for t in per.values] == [(5, 7), (5, 7)]


def test_pow_and_where(emu_backend):
    with precision(64):
        a = np.random.default_rng(0).uniform(0.5, 2.0, (5, 7))
        f = CenteredGrid(a, ZERO_GRADIENT, x=5, y=7, backend=emu_backend)
        np.testing.assert_allclose((f ** 2).numpy(), a ** 2, rtol=1e-15)
        np.testing.assert_allclose((f ** 0.5).numpy(), a ** 0.5, rtol=1e-15)
        with pytest.raises(NotImplementedError):
            f ** f
        mask = CenteredGrid((a > 1.0).astype(np.float64), ZERO_GRADIENT, x=5, y=7, backend=emu_backend)
        np.testing.assert_array_equal(where(mask, f, -1.0).numpy(), np.where(a > 1.0, a, -1.0))
        np.testing.assert_array_equal(where(mask, 3.0, f * 2).numpy(), np.where(a > 1.0, 3.0, 2 * a))
        sphere = Sphere(x=2.5, y=3.5, radius=1.6)
        x, y = np.meshgrid(np.arange(5) + 0.5, np.arange(7) + 0.5, indexing='ij')
        inside = (x - 2.5) ** 2 + (y - 3.5) ** 2 <= 1.6 ** 2
        got = where(sphere, 0.25, f)
        assert got.boundary == f.boundary
        np.testing.assert_array_equal(got.numpy(), np.where(inside, 0.25, a))
        v = StaggeredGrid(1.0, 0, x=5, y=7, backend=emu_backend)
        w = where(sphere, 0.0, v)
        assert w.is_staggered and [tuple(t.shape) for t in w.values] == [tuple(t.shape) for t in v.values] and float(w.values[0].min()) == 0.0


# ---- 3. hand values -----------------------------------------------------------------------------------------------------------------------
def test_hand_values(emu_backend):
    C.check_hand_values(emu_backend)


# ---- 4. backward, element by element ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ['laplace', 'laplace_axes', 'laplace_vector', 'gradient', 'divergence'])
@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_backward_centred(emu_backend, shape, name, op):
    C.check_backward(emu_backend, shape, name, op)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_backward_laplace_staggered(emu_backend, shape, name):
    C.check_backward(emu_backend, shape, name, 'laplace_staggered')


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_backward_curl_staggered(emu_backend, shape, name):
    C.check_backward(emu_backend, shape, name, 'curl_staggered')


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_backward_curl_centred(emu_backend, shape, name):
    C.check_backward(emu_backend, shape, name, 'curl_centred')


def test_backward_entries_accumulate(emu_backend):
    C.check_backward_accumulates(emu_backend)


@pytest.mark.parametrize("chunk", [2, 3])
def test_marching_carries_planes_and_rows_in_registers(emu_backend, chunk):
    C.check_marching_chunks(emu_backend, chunk)


def test_torch_restatements_agree_with_the_numpy_ones():
    """ the differentiated restatements compute what the NumPy ones do (to rounding of float64) """
    R = C.R
    rng = np.random.default_rng(5)
    for shape in ((5, 7), (3, 6, 7)):
        D = len(shape)
        dx = C.dx_of(shape)
        codes = [[R.O.PERIODIC, R.O.PERIODIC], [R.O.CLOSED, R.O.OPEN], [R.O.OPEN, R.O.CLOSED]][:D]
        consts = [(0.0, 0.0), (0.7, 0.0), (0.0, -0.4)][:D]
        a, v = rng.standard_normal((2,) + shape), rng.standard_normal((2, D) + shape)
        w = [1.5, -0.5, 2.0][:D]
        pairs = [(R.t_laplace(torch.tensor(a), dx, codes, consts, w), R.laplace_centered(a, dx, codes, consts, w)[0]),
                 (R.t_gradient(torch.tensor(a), dx, codes, consts), R.gradient_centered(a, dx, codes, consts)[0]),
                 (R.t_divergence(torch.tensor(v), dx, codes, consts), R.divergence_centered(v, dx, codes, consts)[0])]
        if D == 2:
            pairs.append((R.t_curl_centered(torch.tensor(v), codes, consts), R.curl_centered(v, codes, consts)[0]))
            bcv = np.zeros((2, 2, 2))
            bcv[1, 0] = (0.3, -0.2)
            dom = R.O.Domain(shape, (0.3, -1.0), (2.1, 1.5), ((R.O.OPEN, R.O.OPEN), (R.O.CLOSED, R.O.OPEN)), bcv)
            comps = [rng.standard_normal((2,) + dom.comp_shape(d)) for d in range(2)]
            pairs.append((R.t_curl_staggered([torch.tensor(c) for c in comps], dom), R.curl_staggered(comps, dom)[0]))
            for t, n in zip(R.t_laplace_staggered([torch.tensor(c) for c in comps], dom), R.laplace_staggered(comps, dom)[0]):
                pairs.append((t, n))
        for t, n in pairs:
            np.testing.assert_allclose(t.numpy(), n, rtol=0, atol=1e-12 * np.abs(n).max())


# ---- 5. jit_compile ---------------------------------------------------------------------------------------------------------------------------
def test_gray_scott_step_replays_the_eager_bits(emu_backend):
    with precision(32):
        u0, v0 = C.gray_scott_fields(64, emu_backend, 32)
        step = jit_compile(lambda u, v: C.gray_scott(u, v, dt=0.5, **C.MAZE))
        ue, ve, uj, vj = u0, v0, u0, v0
        for _ in range(4):       # the capture and 3 replays
            ue, ve = C.gray_scott(ue, ve, dt=0.5, **C.MAZE)
            uj, vj = step(uj, vj)
            assert np.array_equal(ue.numpy(), uj.numpy()) and np.array_equal(ve.numpy(), vj.numpy())
        ug = CenteredGrid(u0.values[0].clone().requires_grad_(True), PERIODIC, x=64, y=64, backend=emu_backend)
        with pytest.raises(NotImplementedError):
            step(ug, v0)


# ---- 6. the two example steps against NumPy -----------------------------------------------------------------------------------------------------
def _np_laplace(a, dx, mode):
    p = np.pad(a, 1, mode=mode)
    return (p[2:, 1:-1] + p[:-2, 1:-1] - 2 * a) / dx[0] ** 2 + (p[1:-1, 2:] + p[1:-1, :-2] - 2 * a) / dx[1] ** 2


def test_reaction_diffusion_example_step(emu_backend):
    ex = _example("reaction_diffusion")
    with precision(64):
        u, v = C.gray_scott_fields(32, emu_backend, 64)
        un, vn = u.numpy().copy(), v.numpy().copy()
        prm = ex.PATTERNS['coral']
        for _ in range(5):
            u, v = ex.reaction_diffusion(u, v, dt=ex.DT, **prm)
            uvv = un * vn ** 2
            su = prm['du'] * _np_laplace(un, (1.0, 1.0), 'wrap') - uvv + prm['f'] * (1 - un)
            sv = prm['dv'] * _np_laplace(vn, (1.0, 1.0), 'wrap') + uvv - (prm['f'] + prm['k']) * vn
            un, vn = un + ex.DT * su, vn + ex.DT * sv
        assert np.abs(u.numpy() - un).max() <= 1e-12 * np.abs(un).max() and np.abs(v.numpy() - vn).max() <= 1e-12 * np.abs(vn).max()


def test_waves_example_step(emu_backend):
    ex = _example("waves")
    with precision(64):
        n, dt = 32, 0.02     # (a step large enough for the laplace term to matter in 5 steps)
        h_c = h_p = ex.initial_height(n, emu_backend)
        dx = 12.8 / n
        x, y = np.meshgrid((np.arange(n) + 0.5) * dx, (np.arange(n) + 0.5) * dx, indexing='ij')
        hc, hp, t, tn = np.zeros((n, n)), np.zeros((n, n)), 0.0, 0.0
        for _ in range(5):
            h_c, h_p, t = ex.step(h_c, h_p, t, dt=dt, k_damp=0.3)
            inside = (x - (6.4 + np.sin(tn) * 12.8 / 3)) ** 2 + (y - (6.4 - np.cos(tn) * 12.8 / 3)) ** 2 <= 1.0
            hc, hp = np.where(inside, -0.5, hc), np.where(inside, -0.5, hp)
            hc, hp = 2.0 * hc - hp + dt * dt * (_np_laplace(hc, (dx, dx), 'edge') - 0.3 * (hc - hp)), hc
            tn += dt
        assert np.abs(hc).max() > 0.1 and t == tn
        assert np.abs(h_c.numpy() - hc).max() <= 1e-12 * np.abs(hc).max() and np.abs(h_p.numpy() - hp).max() <= 1e-12 * np.abs(hc).max()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(emu_backend):
    s = CenteredGrid(1.0, ZERO_GRADIENT, x=5, y=7, backend=emu_backend)
    v = CenteredGrid((1.0, 2.0), ZERO_GRADIENT, x=5, y=7, backend=emu_backend)
    v3 = CenteredGrid((1.0, 2.0, 3.0), ZERO_GRADIENT, x=3, y=4, z=5, backend=emu_backend)
    st3 = StaggeredGrid(0.5, 0, x=3, y=4, z=5, backend=emu_backend)
    for call in (lambda: laplace(s, order=4), lambda: field.divergence(v, order=4), lambda: field.spatial_gradient(s, at='center', order=4),
                 lambda: laplace(s, weights=s), lambda: curl(v3), lambda: curl(st3), lambda: curl(v, at='center'),
                 lambda: field.spatial_gradient(v, at='center'), lambda: laplace(StaggeredGrid(0.5, 0, x=5, y=7, backend=emu_backend), weights=(1.0, 2.0))):
        with pytest.raises(NotImplementedError):
            call()

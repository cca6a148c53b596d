"""
Centred vector fields (CenteredGrid with a vector axis) on the emulation library: the fused advection by a centred velocity against the fp64
restatement of tests/centered_vector_ref.py, the general path, staggered <-> centres against the oracle, diffusion per component, gradients,
jit_compile, Noise and the Burgers example (examples/grids/Burgers.ipynb; tests/commit/physics/test_advect.py:12-18).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from phiflow_amd.flow import (PERIODIC, ZERO_GRADIENT, Box, CenteredGrid, NotConverged, Obstacle, Solve, StaggeredGrid, advect, assert_close,
                              combine_sides, diffuse, fluid, jit_compile, l2_loss, mean, precision, vec)
from phiflow_amd.noise import Noise
from phiflow_amd.field import _centered_rule

import centered_vector_ref as R
from centered_vector_ref import O
from parity_cases import advect_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXTS = {
    'periodic': PERIODIC,
    'zero_gradient': ZERO_GRADIENT,
    'zero': 0.0,
    'constant': 0.7,
    'mixed': combine_sides(x=(0.7, ZERO_GRADIENT), y=PERIODIC, z=(ZERO_GRADIENT, -0.4)),
}
SHAPES = {2: (13, 7), 3: (13, 7, 5)}


def _ext(name, D):
    e = EXTS[name]
    return combine_sides(x=(0.7, ZERO_GRADIENT), y=PERIODIC) if name == 'mixed' and D == 2 else e


def _bounds(D):
    """ anisotropic cells: dx = 1, 0.5, 2 """
    sizes = [(-1.0, 12.0), (0.0, 3.5), (0.0, 10.0)]
    return Box(**{d: sizes[a] for a, d in enumerate('xyz'[:D])})


def _cvec(arr, ext, bounds, backend):
    """ (B, C, *res) array -> centred vector field (via the public constructor: channel-last, batched when B > 1) """
    D = arr.ndim - 2
    res = dict(zip('xyz', arr.shape[2:]))
    a = np.moveaxis(arr, 1, -1)
    return CenteredGrid(a if arr.shape[0] > 1 else a[0], ext, bounds, backend=backend, **res)


def _rule(f):
    codes, consts = _centered_rule(f, 'test')
    return [list(c) for c in codes], consts


def _amp(arr, consts):
    return max(float(np.abs(arr).max()), max(abs(c) for pair in consts for c in pair), 1e-30)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", ['self', 'separate', 'scalar'])
@pytest.mark.parametrize("ext", list(EXTS))
def test_fused_advection_against_restatement(emu_backend, D, kind, ext):
    rng = np.random.default_rng(hash((D, kind, ext)) % 2 ** 32)
    shape = SHAPES[D]
    bounds = _bounds(D)
    boundary = _ext(ext, D)
    dx = [(u - l) / n for l, u, n in zip(bounds.lower, bounds.upper, shape)]
    for dtype, bits in ((np.float32, 32), (np.float64, 64)):
        for B in (1, 3):
            for disp in (0.3, 2.7):
                with precision(bits):
                    Bv = B if kind == 'self' else 1          # a velocity of batch 1 under a field of batch 3
                    vel_arr = rng.uniform(-1, 1, (Bv, D) + shape).astype(dtype)
                    vel = _cvec(vel_arr, boundary, bounds, emu_backend)
                    dt = disp * min(dx) / float(np.abs(vel_arr).max())
                    if kind == 'self':
                        field, f_arr = vel, vel_arr
                    elif kind == 'separate':
                        f_arr = rng.uniform(-1, 1, (B, D) + shape).astype(dtype)
                        field = _cvec(f_arr, boundary, bounds, emu_backend)
                    else:
                        f_arr = rng.uniform(-1, 1, (B,) + shape).astype(dtype)
                        field = CenteredGrid(f_arr if B > 1 else f_arr[0], boundary, bounds, backend=emu_backend, **dict(zip('xyz', shape)))
                    out = advect.semi_lagrangian(field, vel, dt)
                    codes, consts = _rule(field)
                    ref = R.semi_lagrangian(f_arr if kind != 'scalar' else f_arr[:, None], vel_arr, dt, shape, bounds.lower, bounds.upper, codes, consts)
                    got = out.values.detach().cpu().numpy()
                    if kind == 'scalar':
                        ref = ref[:, 0]
                    else:
                        assert out.is_vector
                    assert got.shape == ref.shape
                    dom = R._dom(shape, bounds.lower, bounds.upper)
                    err = np.abs(got - ref).max() / _amp(f_arr, consts)
                    assert err <= advect_tol(dtype, dom), (dtype, B, disp, err)


@pytest.mark.parametrize("adv", [advect.semi_lagrangian, advect.advect, advect.mac_cormack])
def test_reference_advect_test(emu_backend, adv):
    """ tests/commit/physics/test_advect.py:12-18 with the centred velocity """
    torch.manual_seed(0)
    s = CenteredGrid(Noise(), x=4, y=3, backend=emu_backend)
    v = CenteredGrid(Noise(vector='x,y'), x=4, y=3, backend=emu_backend)
    assert v.is_vector
    assert_close(s, adv(s, v, 0), adv(s, v * 0, 1), abs_tolerance=1e-5)
    assert_close(v, adv(v, v, 0), adv(v, v * 0, 1), abs_tolerance=1e-5)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("ext", ['periodic', 'zero_gradient', 'constant'])
def test_fused_equals_general_path(emu_backend, D, ext):
    """ the fused kernel and the general sampling path (taken when the input requires grad) agree to rounding """
    rng = np.random.default_rng(7)
    shape = SHAPES[D]
    with precision(64):
        arr = rng.uniform(-1, 1, (2, D) + shape)
        v = _cvec(arr, _ext(ext, D), _bounds(D), emu_backend)
        fused = advect.semi_lagrangian(v, v, 0.8)
        vg = v.with_values(v.values.clone().requires_grad_(True))
        general = advect.semi_lagrangian(vg, vg, 0.8)
        np.testing.assert_allclose(general.values.detach().numpy(), fused.values.numpy(), rtol=0, atol=1e-12)
        s = CenteredGrid(rng.uniform(-1, 1, shape), _ext(ext, D), _bounds(D), backend=emu_backend, **dict(zip('xyz', shape)))
        sg = s.with_values(s.values.clone().requires_grad_(True))
        np.testing.assert_allclose(advect.semi_lagrangian(sg, v, 0.8).values.detach().numpy(), advect.semi_lagrangian(s, v, 0.8).values.numpy(),
                                   rtol=0, atol=1e-12)


@pytest.mark.parametrize("ext", ['periodic', 'zero_gradient', 'constant'])
def test_rk4_against_restatement(emu_backend, ext):
    rng = np.random.default_rng(3)
    shape = SHAPES[2]
    bounds = _bounds(2)
    with precision(64):
        arr = rng.uniform(-1, 1, (1, 2) + shape)
        v = _cvec(arr, _ext(ext, 2), bounds, emu_backend)
        out = advect.semi_lagrangian(v, v, 0.9, integrator=advect.rk4)
        codes, consts = _rule(v)
        ref = R.semi_lagrangian(arr, arr, 0.9, shape, bounds.lower, bounds.upper, codes, consts, integrator='rk4')
        np.testing.assert_allclose(out.values.numpy(), ref, rtol=0, atol=1e-12)


def test_staggered_field_by_centred_velocity_raises(emu_backend):
    v = CenteredGrid((1, 0), PERIODIC, x=4, y=3, backend=emu_backend)
    sv = StaggeredGrid(0, PERIODIC, x=4, y=3, backend=emu_backend)
    with pytest.raises(NotImplementedError, match="StaggeredGrid by a centred velocity"):
        advect.semi_lagrangian(sv, v, 1.0)
    with pytest.raises(NotImplementedError, match="CenteredGrid velocity"):
        fluid.make_incompressible(v)
    with pytest.raises(NotImplementedError, match="vector-valued constant"):
        advect.semi_lagrangian(CenteredGrid((1, 0), {'x': vec(x=1, y=0), 'y': 0}, x=4, y=3, backend=emu_backend), v, 1.0)


VEL_BOXES = {
    'periodic': lambda D: O.Domain(SHAPES[D], _bounds(D).lower, _bounds(D).upper, [(O.PERIODIC, O.PERIODIC)] * D),
    'closed': lambda D: O.Domain(SHAPES[D], _bounds(D).lower, _bounds(D).upper, [(O.CLOSED, O.CLOSED)] * D),
    'open': lambda D: O.Domain(SHAPES[D], _bounds(D).lower, _bounds(D).upper, [(O.OPEN, O.OPEN)] * D),
}


def _velocity_boundary(box, D):
    if box == 'periodic':
        return PERIODIC
    if box == 'open':
        return ZERO_GRADIENT
    walls = {'x': vec(**{d: 0.3 * (a + 1) for a, d in enumerate('xyz'[:D])}), 'y': vec(**{d: -0.2 * (a + 1) for a, d in enumerate('xyz'[:D])})}
    if D == 3:
        walls['z'] = vec(x=0.5, y=0.25, z=-0.75)
    return walls


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("box", list(VEL_BOXES))
def test_at_centers_against_oracle(emu_backend, D, box):
    rng = np.random.default_rng(11)
    dom = VEL_BOXES[box](D)
    boundary = _velocity_boundary(box, D)
    with precision(64):
        v = StaggeredGrid(0, boundary, _bounds(D), backend=emu_backend, **dict(zip('xyz', SHAPES[D])))
        comps = [rng.uniform(-1, 1, (2,) + tuple(c.shape[1:])) for c in v.values]
        v = v.with_values([torch.as_tensor(c) for c in comps])
        v.batched = True
        if box == 'closed':     # [axis][side][component]: the wall velocity of each side
            dims = 'xyz'[:D]
            dom.bc_val = np.array([[[float(boundary[da][dc]) for dc in dims] for _ in range(2)] for da in dims])
        c = v.at_centers()
        assert c.is_vector and c.batch_size == 2
        ref = O.staggered_at_centers(comps, dom)
        np.testing.assert_allclose(c.values.numpy(), np.stack(ref, axis=1), rtol=0, atol=1e-14)
        np.testing.assert_array_equal(CenteredGrid(v, boundary if box != 'closed' else 0, _bounds(D), backend=emu_backend,
                                                   **dict(zip('xyz', SHAPES[D]))).values.numpy(),
                                      c.values.numpy())


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("box,ext", [('periodic', 'periodic'), ('closed', 'zero_gradient'), ('closed', 'constant'), ('open', 'zero_gradient'),
                                     ('open', 'constant')])
def test_centred_to_faces_against_oracle(emu_backend, D, box, ext):
    rng = np.random.default_rng(5)
    dom = VEL_BOXES[box](D)
    with precision(64):
        arr = rng.uniform(-1, 1, (2, D) + SHAPES[D])
        cv = _cvec(arr, _ext(ext, D), _bounds(D), emu_backend)
        target = StaggeredGrid(0, {'periodic': PERIODIC, 'closed': 0, 'open': ZERO_GRADIENT}[box], _bounds(D), backend=emu_backend,
                               **dict(zip('xyz', SHAPES[D])))
        faces = cv @ target
        assert faces.is_staggered
        codes, consts = _rule(cv)
        for d in range(D):
            ref = O.centered_to_staggered(np.ascontiguousarray(arr[:, d]), dom, codes, consts)[d]
            np.testing.assert_allclose(faces.values[d].numpy(), ref, rtol=0, atol=1e-14)
        same = StaggeredGrid(cv, target.boundary, _bounds(D), backend=emu_backend, **dict(zip('xyz', SHAPES[D])))
        for a, b in zip(same.values, faces.values):
            np.testing.assert_array_equal(a.numpy(), b.numpy())


def test_constructors_access_and_arithmetic(emu_backend):
    rng = np.random.default_rng(1)
    arr = rng.uniform(-1, 1, (5, 4, 2)).astype(np.float32)
    v = CenteredGrid(arr, PERIODIC, x=5, y=4, backend=emu_backend)
    assert v.is_vector and not v.batched
    np.testing.assert_array_equal(v.numpy(), arr)
    np.testing.assert_array_equal(v['y'].numpy(), arr[..., 1])
    assert not v['y'].is_vector
    batched = CenteredGrid(np.stack([arr, 2 * arr]), PERIODIC, x=5, y=4, backend=emu_backend)
    assert batched.batched and batched.numpy().shape == (2, 5, 4, 2)
    np.testing.assert_array_equal(CenteredGrid(torch.as_tensor(arr), PERIODIC, x=5, y=4, backend=emu_backend).numpy(), arr)
    np.testing.assert_allclose((v * (1, -1)).numpy(), arr * np.array([1, -1], np.float32))
    np.testing.assert_allclose((v + v * 2 - 1).numpy(), 3 * arr - 1, rtol=1e-6)
    np.testing.assert_allclose((v / 2).numpy(), arr / 2)
    np.testing.assert_allclose(mean(v).numpy(), arr.reshape(-1, 2).mean(0), rtol=1e-5)
    const = CenteredGrid((1.0, -2.0), 0, x=3, y=2, backend=emu_backend)
    np.testing.assert_array_equal(const.numpy(), np.broadcast_to([1.0, -2.0], (3, 2, 2)))
    np.testing.assert_array_equal(CenteredGrid(vec(x=1.0, y=-2.0), 0, x=3, y=2, backend=emu_backend).numpy(), const.numpy())
    fn = CenteredGrid(lambda x, y: vec(x=x, y=-y), 0, x=3, y=2, backend=emu_backend)
    np.testing.assert_allclose(fn.numpy()[..., 0], np.broadcast_to(np.arange(3)[:, None] + 0.5, (3, 2)))
    # the inputs that keep today's meaning: a batch of scalar fields
    assert not CenteredGrid([np.zeros((3, 2)), np.ones((3, 2))], 0, x=3, y=2, backend=emu_backend).is_vector
    assert not CenteredGrid(np.zeros((2, 2, 2)), 0, x=2, y=2, backend=emu_backend).is_vector
    # lazy scalar * vector: stays lazy on a scalar, becomes a real vector field resampled to a centred vector target
    s = CenteredGrid(rng.uniform(0, 1, (3, 2)), 0, x=3, y=2, backend=emu_backend)
    lazy = s * (0, 0.1)
    assert lazy.vector_scale == [0.0, 0.1] and not lazy.is_vector
    real = lazy @ const
    assert real.is_vector
    np.testing.assert_allclose(real.numpy()[..., 1], 0.1 * s.numpy(), rtol=1e-6)
    with pytest.raises(NotImplementedError):
        lazy @ s


def _sparse_implicit(s, k, dt, dom, codes, consts):
    """ direct solve of sharpen(x) = y for the affine sharpen(x) = explicit(x, k, -dt) (one batch entry) """
    n = s.size
    sharpen = lambda x: O.diffuse_explicit_centered(x.reshape((1,) + s.shape), k, -dt, dom, codes, consts)[0].reshape(-1)
    bias = sharpen(np.zeros(n))
    A = np.stack([sharpen(e) - bias for e in np.eye(n)], axis=1)
    return np.linalg.solve(A, s.reshape(-1) - bias).reshape(s.shape)


@pytest.mark.parametrize("ext", ['periodic', 'zero_gradient', 'constant'])
def test_diffusion_per_component(emu_backend, ext):
    rng = np.random.default_rng(2)
    shape = (6, 5)
    bounds = _bounds(2)
    dom = R._dom(shape, bounds.lower, bounds.upper)
    with precision(64):
        arr = rng.uniform(-1, 1, (2, 2) + shape)
        v = _cvec(arr, _ext(ext, 2), bounds, emu_backend)
        codes, consts = _rule(v)
        ex = diffuse.explicit(v, 0.1, 1.0)
        assert ex.is_vector
        for b in range(2):
            for c in range(2):
                ref = O.diffuse_explicit_centered(arr[b:b + 1, c], 0.1, 1.0, dom, codes, consts)[0]
                np.testing.assert_allclose(ex.values[b, c].numpy(), ref, rtol=0, atol=1e-13)
        im = diffuse.implicit(v, 0.5, 1.0, Solve('CG', 1e-12, 0, max_iterations=500))
        assert im.is_vector and len(im.solve_info.iterations) == 4      # one solve per (batch entry, component)
        for b in range(2):
            for c in range(2):
                np.testing.assert_allclose(im.values[b, c].numpy(), _sparse_implicit(arr[b, c], 0.5, 1.0, dom, codes, consts), rtol=0, atol=1e-9)
        # per-axis and Field diffusivities of batch B are expanded to B * C
        kfield = CenteredGrid(rng.uniform(0.05, 0.1, (2,) + shape), ZERO_GRADIENT, bounds, backend=emu_backend, x=6, y=5)
        fx = diffuse.explicit(v, kfield, 1.0)
        for c in range(2):
            solo = diffuse.explicit(CenteredGrid(arr[:, c], _ext(ext, 2), bounds, backend=emu_backend, x=6, y=5), kfield, 1.0)
            np.testing.assert_array_equal(fx.values[:, c].numpy(), solo.values.numpy())
        # a component that needs more iterations than allowed fails the whole call
        arr2 = arr.copy()
        arr2[:, 0] = 0.0
        with pytest.raises(NotConverged):
            diffuse.implicit(_cvec(arr2, _ext(ext, 2), bounds, emu_backend), 0.5, 1.0, Solve('CG', 1e-12, 0, max_iterations=2))


def _fd_check(fn, x0, eps=1e-6, rtol=1e-6, picks=8, seed=0):
    x = x0.clone().requires_grad_(True)
    fn(x).backward()
    g = x.grad.numpy().reshape(-1)
    rng = np.random.default_rng(seed)
    for i in rng.choice(g.size, size=picks, replace=False):
        xp, xm = x0.clone().reshape(-1), x0.clone().reshape(-1)
        xp[i] += eps
        xm[i] -= eps
        fd = (fn(xp.reshape(x0.shape)).item() - fn(xm.reshape(x0.shape)).item()) / (2 * eps)
        assert abs(fd - g[i]) <= rtol * max(1.0, abs(fd)) + 1e-7, (i, fd, g[i])


def test_gradients_against_finite_differences(emu_backend):
    rng = np.random.default_rng(4)
    with precision(64):
        arr = rng.uniform(-1, 1, (1, 2, 6, 5))
        v0 = _cvec(arr, PERIODIC, _bounds(2), emu_backend)
        s0 = CenteredGrid(rng.uniform(-1, 1, (6, 5)), ZERO_GRADIENT, _bounds(2), backend=emu_backend, x=6, y=5)

        def self_adv(t):
            v = v0.with_values(t)
            return l2_loss(advect.semi_lagrangian(v, v, 0.6))

        def scalar_adv(t):
            return l2_loss(advect.semi_lagrangian(s0, v0.with_values(t), 0.6))

        _fd_check(self_adv, v0.values.detach())
        _fd_check(scalar_adv, v0.values.detach(), seed=1)
        sv = StaggeredGrid(0, 0, _bounds(2), backend=emu_backend, x=6, y=5)
        comps = [torch.as_tensor(rng.uniform(-1, 1, c.shape)) for c in sv.values]

        def centres(t):
            return l2_loss(sv.with_values([t, comps[1]]).at_centers())

        _fd_check(centres, comps[0])


def _burgers_module():
    spec = importlib.util.spec_from_file_location("burgers_example", os.path.join(ROOT, "examples", "burgers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_jit_burgers_step_replays_eager_bits(emu_backend):
    mod = _burgers_module()
    torch.manual_seed(0)
    v0 = mod.initial_velocity(16, backend=emu_backend)
    eager = v0
    for _ in range(3):
        eager = mod.step(eager)
    jitted = jit_compile(mod.step)
    out = v0
    for _ in range(3):
        out = jitted(out)
    assert out.is_vector
    np.testing.assert_array_equal(out.numpy(), eager.numpy())


def test_burgers_example_maximum_principle(emu_backend):
    mod = _burgers_module()
    torch.manual_seed(1)
    v = mod.initial_velocity(32, backend=emu_backend)
    e0 = mod.kinetic_energy(v)
    m0 = mod.max_abs(v)
    for _ in range(10):
        v = mod.step(v)
        m = mod.max_abs(v)
        assert all(a <= b * (1 + 1e-4) for a, b in zip(m, m0)), (m, m0)
    assert mod.kinetic_energy(v) < e0


def test_noise_statistics(emu_backend):
    torch.manual_seed(3)
    s = CenteredGrid(Noise(), PERIODIC, x=32, y=24, backend=emu_backend)
    a = s.numpy().astype(np.float64)
    assert abs(a.mean()) < 1e-6 and abs(a.std() - 1) < 1e-5
    v = CenteredGrid(Noise(scale=10, smoothness=1, vector='x,y'), PERIODIC, x=32, y=24, backend=emu_backend)
    b = v.numpy().astype(np.float64)
    assert abs(b.mean()) < 1e-6 and abs(b.std() - 1) < 1e-5        # over all non-batch dims, the vector axis included
    # no energy at k^2 <= 0.1 (k = fftfreq(n, size) * n * scale)
    for c in range(2):
        spec = np.abs(np.fft.fftn(b[..., c]))
        kx = np.fft.fftfreq(32, 32.0) * 32 * 10
        ky = np.fft.fftfreq(24, 24.0) * 24 * 10
        k2 = kx[:, None] ** 2 + ky[None, :] ** 2
        assert spec[k2 <= 0.1].max() < 1e-4 * spec.max()
    corr = np.corrcoef(b[..., 0].ravel(), b[..., 1].ravel())[0, 1]
    assert abs(corr) < 0.3
    torch.manual_seed(3)
    np.testing.assert_array_equal(CenteredGrid(Noise(), PERIODIC, x=32, y=24, backend=emu_backend).numpy(), s.numpy())
    sg = StaggeredGrid(Noise(), 0, x=8, y=6, backend=emu_backend)
    assert [tuple(c.shape) for c in sg.numpy()] == [(7, 6), (8, 5)]
    nb = CenteredGrid(Noise(vector='x,y', batch=3), PERIODIC, x=8, y=6, backend=emu_backend)
    assert nb.batched and nb.numpy().shape == (3, 8, 6, 2)


def test_obstacles_with_centred_velocity_raise(emu_backend):
    """ obstacles meet staggered velocities only: a centred velocity is refused before any kernel sees its (B, D, *res) tensor """
    box = Obstacle(Box(x=(1, 3), y=(1, 2)))
    for B, ext in ((1, ZERO_GRADIENT), (2, PERIODIC)):
        v = _cvec(np.ones((B, 2, 4, 3)), ext, Box(x=4, y=3), emu_backend)
        with pytest.raises(NotImplementedError, match="obstacles with a CenteredGrid velocity"):
            fluid.apply_boundary_conditions(v, [box])
    assert fluid.apply_boundary_conditions(v, ()) is v          # no obstacles: nothing to do


def test_one_dimensional_vector_fields_raise(emu_backend):
    with pytest.raises(NotImplementedError, match="1-D grids"):
        CenteredGrid(Noise(vector='x'), PERIODIC, x=64, backend=emu_backend)
    with pytest.raises(NotImplementedError, match="1-D grids"):
        CenteredGrid((1.0,), PERIODIC, x=8, backend=emu_backend)


def test_one_cell_between_constant_sides(emu_backend):
    """ a centred field may have one cell between two constant sides (the C layer's grid view has no face bookkeeping for it) """
    rng = np.random.default_rng(21)
    shape = (1, 7)
    bounds = Box(x=(0, 2), y=(0, 3.5))
    ext = combine_sides(x=0.7, y=ZERO_GRADIENT)
    with precision(64):
        arr = rng.uniform(-1, 1, (2, 2) + shape)
        v = _cvec(arr, ext, bounds, emu_backend)
        out = advect.semi_lagrangian(v, v, 0.9)
        codes, consts = _rule(v)
        ref = R.semi_lagrangian(arr, arr, 0.9, shape, bounds.lower, bounds.upper, codes, consts)
        np.testing.assert_allclose(out.values.numpy(), ref, rtol=0, atol=1e-12)


def _batch_points(points, B):
    return [np.broadcast_to(p[None], (B,) + p.shape) for p in points]


def test_resample_between_different_grids(emu_backend):
    """ at_centers / centred vector -> faces onto another grid go through the general gather (resample_general) """
    rng = np.random.default_rng(22)
    bounds = Box(x=(0, 8), y=(0, 3))
    src_dom = O.Domain((8, 6), bounds.lower, bounds.upper, [(O.CLOSED, O.CLOSED)] * 2)
    dst_dom = O.Domain((5, 4), bounds.lower, bounds.upper, [(O.CLOSED, O.CLOSED)] * 2)
    with precision(64):
        sv = StaggeredGrid(0, 0, bounds, backend=emu_backend, x=8, y=6)
        comps = [rng.uniform(-1, 1, (2,) + tuple(c.shape[1:])) for c in sv.values]
        sv = sv.with_values([torch.as_tensor(c) for c in comps])
        sv.batched = True
        target = CenteredGrid((0.0, 0.0), 0, bounds, backend=emu_backend, x=5, y=4)
        got = sv @ target
        assert got.is_vector and got.resolution == {'x': 5, 'y': 4}
        ref = O.sample_staggered_at(comps, src_dom, _batch_points(O.cell_positions(dst_dom, np.float64), 2))
        np.testing.assert_allclose(got.values.numpy(), np.stack(ref, axis=1), rtol=0, atol=1e-13)
        arr = rng.uniform(-1, 1, (2, 2, 8, 6))
        cv = _cvec(arr, ZERO_GRADIENT, bounds, emu_backend)
        faces = cv @ StaggeredGrid(0, 0, bounds, backend=emu_backend, x=5, y=4)
        codes, consts = _rule(cv)
        for d in range(2):
            r = O.sample_centered_at(np.ascontiguousarray(arr[:, d]), src_dom, codes, consts, _batch_points(O.face_positions(d, dst_dom, np.float64), 2))
            np.testing.assert_allclose(faces.values[d].numpy(), r, rtol=0, atol=1e-13)


def test_centred_to_faces_of_other_periodicity(emu_backend):
    """ a periodic centred vector sampled at the faces of a closed box: the general gather with the field's own (periodic) rule """
    rng = np.random.default_rng(23)
    bounds = _bounds(2)
    dom = O.Domain(SHAPES[2], bounds.lower, bounds.upper, [(O.CLOSED, O.CLOSED)] * 2)
    with precision(64):
        arr = rng.uniform(-1, 1, (1, 2) + SHAPES[2])
        cv = _cvec(arr, PERIODIC, bounds, emu_backend)
        faces = StaggeredGrid(cv, 0, bounds, backend=emu_backend, **dict(zip('xyz', SHAPES[2])))
        codes, consts = _rule(cv)
        for d in range(2):
            r = O.sample_centered_at(np.ascontiguousarray(arr[:, d]), dom, codes, consts, _batch_points(O.face_positions(d, dom, np.float64), 1))
            np.testing.assert_allclose(faces.values[d].numpy(), r, rtol=0, atol=1e-13)


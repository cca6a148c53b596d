"""
Shared cases of the differential-operator tests (tests/test_diffops_emu.py on the emulation library, tests/test_gpu_diffops.py on the device):
every check takes the backend it runs on. References: tests/diffops_ref.py (float64).

Bound of the element-wise checks, derived, not measured: an output is a sum of at most 2 D + 1 products, each with one rounded weight, so
|got - exact| <= (2 D + 6) eps(T) S with S = sum |w_k U_k| of that element (the float64 reference carries the same bound in eps(float64)).
"""
import zlib

import numpy as np
import torch

from phiflow_amd import field
from phiflow_amd.flow import PERIODIC, ZERO_GRADIENT, Box, CenteredGrid, StaggeredGrid, combine_sides, precision, vec

import diffops_ref as R
from diffops_ref import O

SHAPES = [(5, 7), (9, 66), (6, 130), (3, 6, 70), (9, 8, 7), (2, 5, 65)]
SHAPES_2D = [s for s in SHAPES if len(s) == 2]
CENTRED_EXTS = ['periodic', 'zero_gradient', 'zero', 'constant', 'mixed']
STAGGERED_EXTS = CENTRED_EXTS + ['lid']
DTYPES = ((np.float32, 32), (np.float64, 64))
BATCHES = (1, 3)


def ext(name, D):
    if name == 'periodic':
        return PERIODIC
    if name == 'zero_gradient':
        return ZERO_GRADIENT
    if name == 'zero':
        return 0.0
    if name == 'constant':
        return 0.7
    if name == 'mixed':
        return combine_sides(x=PERIODIC, y=(0.7, ZERO_GRADIENT)) if D == 2 else combine_sides(x=PERIODIC, y=(0.7, ZERO_GRADIENT), z=(ZERO_GRADIENT, -0.4))
    assert name == 'lid'
    return {'x': 0, 'y-': 0, 'y+': vec(x=1, y=0)} if D == 2 else {'x': 0, 'y': 0, 'z-': 0, 'z+': vec(x=1, y=0, z=0)}


def bounds(D):
    """ non-unit, anisotropic cells """
    sizes = [(0.3, 2.1), (-1.0, 1.5), (0.0, 3.0)]
    return Box(**{d: sizes[a] for a, d in enumerate('xyz'[:D])})


def res_kw(shape):
    return dict(zip('xyz', shape))


def dx_of(shape):
    b = bounds(len(shape))
    return [(u - l) / n for l, u, n in zip(b.lower, b.upper, shape)]


def rng_for(*key):
    """ a generator seeded by the case's key alone (crc32 of its repr: the same inputs in every run, process and xdist worker) """
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def eps(dtype):
    return float(np.finfo(dtype).eps)


def centred_scalar(arr, boundary, backend):
    """ (B, *res) array -> centred scalar field """
    return CenteredGrid(arr if arr.shape[0] > 1 else arr[0], boundary, bounds(arr.ndim - 1), backend=backend, **res_kw(arr.shape[1:]))


def centred_vector(arr, boundary, backend):
    """ (B, D, *res) array -> centred vector field (the constructor takes channel-last) """
    a = np.moveaxis(arr, 1, -1)
    return CenteredGrid(a if arr.shape[0] > 1 else a[0], boundary, bounds(arr.ndim - 2), backend=backend, **res_kw(arr.shape[2:]))


def staggered(comps, boundary, shape, backend):
    return StaggeredGrid([c if c.shape[0] > 1 else c[0] for c in comps], boundary, bounds(len(shape)), backend=backend, **res_kw(shape))


_P, _C, _O = O.PERIODIC, O.CLOSED, O.OPEN       # wrap / constant / edge copy


def rule(name, D):
    """ (codes[D][2], consts[D][2]) of the centred extrapolation `ext(name, D)`, written out (not asked of the package under test) """
    if name == 'mixed':
        return [[_P, _P], [_C, _O], [_O, _C]][:D], [(0.0, 0.0), (0.7, 0.0), (0.0, -0.4)][:D]
    code, const = {'periodic': (_P, 0.0), 'zero_gradient': (_O, 0.0), 'zero': (_C, 0.0), 'constant': (_C, 0.7)}[name]
    return [[code, code] for _ in range(D)], [(const, const)] * D


def domain(name, shape):
    """ oracle Domain of a staggered field with `ext(name, D)`, written out: bc_val[axis][side][component] """
    D = len(shape)
    b = bounds(D)
    val = np.zeros((D, 2, D))
    if name == 'lid':           # closed box, the upper side of the last axis moves along x
        codes = [[_C, _C] for _ in range(D)]
        val[D - 1, 1, 0] = 1.0
    else:
        codes, consts = rule(name, D)
        for a in range(D):
            for side in range(2):
                val[a, side, :] = consts[a][side]
    return O.Domain(shape, b.lower, b.upper, [tuple(c) for c in codes], val)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def assert_elementwise(got, ref, S, dtype, D, what):
    """ |got - ref| <= (2 D + 6) eps S for EVERY element """
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = (2 * D + 6) * eps(dtype) * S
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst ratio {float((err[bad] / np.maximum(bound[bad], 1e-300)).max()):.3g}"


def configurations(shape, name):
    """ (dtype, bits, batch, rng) of every case of one (shape, extrapolation) """
    for dtype, bits in DTYPES:
        for B in BATCHES:
            yield dtype, bits, B, rng_for(shape, name, bits, B)


# ---- check 1: forward, element by element ---------------------------------------------------------------------------------------------------
def laplace_weight_forms(D):
    """ (weights argument, axes argument, per-axis factors): None, a number, a per-axis vector, an axis subset """
    per_axis = [1.5, -0.5, 2.0][:D]
    subset = ['x', 'z'][:D - 1] if D == 3 else ['y']
    return [(None, None, [1.0] * D), (0.3, None, [0.3] * D), (vec(**dict(zip('xyz', per_axis))), None, per_axis),
            (None, subset, [1.0 if d in subset else 0.0 for d in 'xyz'[:D]]), (tuple(per_axis), ','.join(subset), [w if d in subset else 0.0 for w, d in zip(per_axis, 'xyz')])]


def check_laplace_centred(backend, shape, name):
    D = len(shape)
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            a = rng.standard_normal((B,) + shape).astype(dtype)
            u = centred_scalar(a, ext(name, D), backend)
            codes, consts = rule(name, D)
            for weights, axes, w in laplace_weight_forms(D):
                ref, S = R.laplace_centered(a, dx_of(shape), codes, consts, w)
                out = field.laplace(u, axes=axes, weights=weights) if axes is not None else field.laplace(u, weights=weights)
                assert not out.is_staggered and not out.is_vector and out.resolution == u.resolution
                assert_elementwise(host(out.values), ref, S, dtype, D, f"laplace {shape} {name} {dtype.__name__} B={B} w={w}")
            # tie to the oracle: laplace = diffuse_explicit_centered(u, 1, 1) - u
            ref, _ = R.laplace_centered(a, dx_of(shape), codes, consts, [1.0] * D)
            dom = O.Domain(shape, bounds(D).lower, bounds(D).upper, [(0, 0)] * D)
            a64 = a.astype(np.float64)
            tie = O.diffuse_explicit_centered(a64, 1.0, 1.0, dom, codes, consts) - a64
            assert np.abs(tie - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
            # every component of a centred vector field, the (B * C, *res) view
            av = rng.standard_normal((B, D) + shape).astype(dtype)
            uv = centred_vector(av, ext(name, D), backend)
            ref, S = R.laplace_centered(av.reshape((B * D,) + shape), dx_of(shape), codes, consts, [1.0] * D)
            out = uv.laplace()
            assert out.is_vector
            assert_elementwise(host(out.values), ref.reshape(av.shape), S.reshape(av.shape), dtype, D, f"vector laplace {shape} {name}")


def check_laplace_staggered(backend, shape, name):
    D = len(shape)
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            proto = StaggeredGrid(0, ext(name, D), bounds(D), backend=backend, **res_kw(shape))
            comps = [rng.standard_normal((B,) + s).astype(dtype) for s in proto.component_shapes]
            v = staggered(comps, ext(name, D), shape, backend)
            dom = domain(name, shape)
            for weight in (None, -0.7):
                refs, Ss = R.laplace_staggered(comps, dom, 1.0 if weight is None else weight)
                out = field.laplace(v, weights=weight)
                assert out.is_staggered
                expect = v.with_values([torch.as_tensor(r) for r in refs]).with_boundary(out.boundary)      # (the result's face layout: BOUNDARY -> ZERO drops faces)
                scale = v.with_values([torch.as_tensor(s) for s in Ss]).with_boundary(out.boundary)
                for c in range(D):
                    assert_elementwise(host(out.values[c]), expect.values[c].numpy(), scale.values[c].numpy(), dtype, D, f"staggered laplace {shape} {name} c={c}")
            refs, _ = R.laplace_staggered(comps, dom)
            for c in range(D):
                tie = O.laplace_component(comps[c].astype(np.float64), c, dom)
                assert np.abs(tie - refs[c]).max() <= 1e-12 * max(np.abs(refs[c]).max(), 1e-300)


def check_gradient(backend, shape, name):
    D = len(shape)
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            a = rng.standard_normal((B,) + shape).astype(dtype)
            u = centred_scalar(a, ext(name, D), backend)
            ref, S = R.gradient_centered(a, dx_of(shape), *rule(name, D))
            out = field.spatial_gradient(u, at='center')
            assert out.is_vector and out.resolution == u.resolution
            assert_elementwise(host(out.values), ref, S, dtype, D, f"gradient {shape} {name} {dtype.__name__} B={B}")


def check_divergence(backend, shape, name):
    D = len(shape)
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            a = rng.standard_normal((B, D) + shape).astype(dtype)
            v = centred_vector(a, ext(name, D), backend)
            ref, S = R.divergence_centered(a, dx_of(shape), *rule(name, len(shape)))
            out = field.divergence(v)
            assert not out.is_vector and not out.is_staggered
            assert_elementwise(host(out.values), ref, S, dtype, D, f"divergence {shape} {name} {dtype.__name__} B={B}")
            assert_elementwise(host(v.divergence().values), ref, S, dtype, D, "Field.divergence")


def check_curl_staggered(backend, shape, name):
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            proto = StaggeredGrid(0, ext(name, 2), bounds(2), backend=backend, **res_kw(shape))
            comps = [rng.standard_normal((B,) + s).astype(dtype) for s in proto.component_shapes]
            v = staggered(comps, ext(name, 2), shape, backend)
            ref, S = R.curl_staggered(comps, domain(name, shape))
            out = field.curl(v)
            assert tuple(out.values.shape) == (B, shape[0] + 1, shape[1] + 1)
            assert_elementwise(host(out.values), ref, S, dtype, 2, f"staggered curl {shape} {name} {dtype.__name__} B={B}")


def check_curl_centred(backend, shape, name):
    for dtype, bits, B, rng in configurations(shape, name):
        with precision(bits):
            a = rng.standard_normal((B, 2) + shape).astype(dtype)
            v = centred_vector(a, ext(name, 2), backend)
            ref, S = R.curl_centered(a, *rule(name, len(shape)))
            out = v.curl()
            assert tuple(out.values.shape) == (B, shape[0] + 1, shape[1] + 1)
            assert_elementwise(host(out.values), ref, S, dtype, 2, f"centred curl {shape} {name} {dtype.__name__} B={B}")


# ---- check 3: hand values -------------------------------------------------------------------------------------------------------------------
def check_hand_values(backend):
    with precision(64):
        b = Box(x=(0.3, 2.1), y=(-1.0, 1.5))
        # rigid rotation v = (-y, x): curl = 2 at every interior corner of the staggered grid, 2 (dx + dy) in the centred form
        vs = StaggeredGrid(lambda x, y: (-y, x), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        c = vs.curl().numpy()
        assert c.shape == (7, 6)
        np.testing.assert_allclose(c[1:-1, 1:-1], 2.0, rtol=0, atol=1e-12)
        vc = CenteredGrid(lambda x, y: vec(x=-y, y=x), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        dx, dy = vc.dx
        np.testing.assert_allclose(vc.curl().numpy()[1:-1, 1:-1], 2.0 * (dx + dy), rtol=0, atol=1e-12)
        # divergence of (x, y) = 2, laplace of x^2 + y^2 = 4 in the interior
        d = CenteredGrid(lambda x, y: vec(x=x, y=y), ZERO_GRADIENT, b, x=6, y=5, backend=backend).divergence().numpy()
        np.testing.assert_allclose(d[1:-1, 1:-1], 2.0, rtol=0, atol=1e-12)
        lap = CenteredGrid(lambda x, y: x ** 2 + y ** 2, ZERO_GRADIENT, b, x=6, y=5, backend=backend).laplace().numpy()
        np.testing.assert_allclose(lap[1:-1, 1:-1], 4.0, rtol=0, atol=1e-11)


# ---- check 4: backward, element by element ----------------------------------------------------------------------------------------------------
def _check_vjp(backend, dtype, D, arrays, make_field, apply, t_fn, what, restrict=None):
    """ arrays: the inputs; make_field(leaf tensors) -> Field; apply(Field) -> Field; t_fn(*torch inputs, absolute=...) the float64 restatement
    (restrict: maps its outputs to the faces the result stores). The input gradients ACCUMULATE into non-zero `.grad` buffers: the seed is
    +-S per element, so the one extra rounding of the accumulation, eps / 2 (|seed| + |grad|) <= eps S, stays inside the bound's margin
    (the transposed stencil itself needs at most (2 D + 2) eps / 2 S of the (2 D + 6) eps S). """
    rng = rng_for(what, 'gout')
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    leaves = [torch.tensor(a, dtype=tdt, device=backend.device, requires_grad=True) for a in arrays]
    out = apply(make_field(leaves))
    outs = list(out.values) if out.is_staggered else [out.values]
    gouts = [rng.standard_normal(tuple(o.shape)).astype(dtype) for o in outs]
    restrict = restrict or (lambda ys: ys)

    def listed(y):
        return restrict(list(y) if isinstance(y, (list, tuple)) else [y])
    ref = R.vjp(lambda *xs: listed(t_fn(*xs, absolute=False)), arrays, gouts)
    S = R.vjp(lambda *xs: listed(t_fn(*xs, absolute=True)), arrays, [np.abs(g) for g in gouts])
    seeds = [torch.tensor((np.where(rng.random(s.shape) < 0.5, -1.0, 1.0) * s).astype(dtype), device=backend.device) for s in S]
    for t, sd in zip(leaves, seeds):
        t.grad = sd.clone()
    torch.autograd.backward(outs, [torch.tensor(g, device=backend.device) for g in gouts])
    for k, (t, sd, r, s) in enumerate(zip(leaves, seeds, ref, S)):
        assert_elementwise(host(t.grad), host(sd) + r, s, dtype, D, f"{what} input {k}")


def _stored_faces_restriction(f_old, new_boundary):
    """ restatement outputs on the input's face layout -> the faces a field with `new_boundary` stores (Field.with_boundary's slicing) """
    def restrict(ys):
        out = []
        for d, (dim, y) in enumerate(zip(f_old.dims, ys)):
            lo_old, up_old = f_old.boundary.valid_outer_faces(dim)
            lo_new, up_new = new_boundary.valid_outer_faces(dim)
            assert lo_old >= lo_new and up_old >= up_new
            start = int(lo_old) - int(lo_new)
            out.append(y.narrow(1 + d, start, y.shape[1 + d] - start - (int(up_old) - int(up_new))))
        return out
    return restrict


def check_backward_accumulates(backend):
    """ the *_backward entries (and adjoint = 1) add to their outputs: two calls into zeroed buffers give exactly twice one call (x + x is exact) """
    from phiflow_amd.field import _cell_grid
    rng = rng_for('accumulate')
    shape = (5, 66)
    with precision(32):
        u = centred_scalar(rng.standard_normal((2,) + shape).astype(np.float32), ext('mixed', 2), backend)
        v = centred_vector(rng.standard_normal((2, 2) + shape).astype(np.float32), ext('mixed', 2), backend)
        proto = StaggeredGrid(0, ext('mixed', 2), bounds(2), backend=backend, **res_kw(shape))
        vs = staggered([rng.standard_normal((2,) + s).astype(np.float32) for s in proto.component_shapes], ext('mixed', 2), shape, backend)
        codes, consts = rule('mixed', 2)
        grid = _cell_grid(u)
        c = backend.ctx
        corner = torch.tensor(rng.standard_normal((2, shape[0] + 1, shape[1] + 1)).astype(np.float32), device=backend.device)
        P = lambda ts: [t.data_ptr() for t in ts]
        zeros = lambda *shapes: [torch.zeros(sh, dtype=torch.float32, device=backend.device) for sh in shapes]
        faces = [(2, shape[0] + 1, shape[1]), (2, shape[0], shape[1] + 1)]           # all faces, as Field.curl bakes them
        calls = [
            (lambda o: c.gradient_centered_backward(grid, codes, v.values.data_ptr(), o[0].data_ptr(), backend.stream()), [tuple(u.values.shape)]),
            (lambda o: c.divergence_centered_backward(grid, codes, u.values.data_ptr(), o[0].data_ptr(), backend.stream()), [tuple(v.values.shape)]),
            (lambda o: c.field_laplace_centered(grid, u.values.data_ptr(), codes, consts, [1.0, 2.0], o[0].data_ptr(), True, backend.stream()), [tuple(u.values.shape)]),
            (lambda o: c.curl_2d_backward(grid, False, codes, corner.data_ptr(), o[0].data_ptr(), 0, backend.stream()), [tuple(v.values.shape)]),
            (lambda o: c.curl_2d_backward(grid, True, codes, corner.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), backend.stream()), faces),
            (lambda o: c.field_laplace(vs.grid_struct(), P(vs.values), P(o), 0.7, True, backend.stream()), [tuple(t.shape) for t in vs.values]),
        ]
        for call, shapes in calls:
            once, twice = zeros(*shapes), zeros(*shapes)
            call(once)
            call(twice)
            call(twice)
            for a1, a2 in zip(once, twice):
                assert float(a1.abs().max()) > 0 and torch.equal(a2, 2 * a1)


CHUNK_SHAPES_3D = [(9, 8, 7), (3, 6, 70)]
CHUNK_EXTS = ['periodic', 'zero_gradient', 'constant', 'mixed']


def check_marching_chunks(backend, chunk):
    """ the register carry of the marching loops: at the shapes of these tests the launch plan gives every workgroup ONE plane (one row of
    corners), so the planes per workgroup are set by hand (tuning family 0) -- chunk 2 and 3 split 9 and 3 planes, and 6 / 7 / 10 rows of corners, into
    whole and partial chunks. Forward and backward of the centred gradient and divergence (cgrad / cdiv kernels, both directions each) and of both curls. """
    backend.ctx.set_tuning_kernel(0, 0, 0, chunk)
    try:
        for name in CHUNK_EXTS:
            for shape in CHUNK_SHAPES_3D:
                check_gradient(backend, shape, name)
                check_divergence(backend, shape, name)
                check_backward(backend, shape, name, 'gradient')
                check_backward(backend, shape, name, 'divergence')
            for shape in SHAPES_2D:
                check_curl_staggered(backend, shape, name)
                check_curl_centred(backend, shape, name)
        check_curl_staggered(backend, (9, 66), 'lid')
        check_backward(backend, (9, 66), 'mixed', 'curl_staggered')
        check_backward(backend, (9, 66), 'mixed', 'curl_centred')
    finally:
        backend.ctx.set_tuning_kernel(0, 0, 0, 0)


def check_backward(backend, shape, name, op):
    """ op: 'laplace' | 'laplace_axes' | 'laplace_vector' | 'laplace_staggered' | 'gradient' | 'divergence' | 'curl_staggered' | 'curl_centred' """
    D = len(shape)
    dx = dx_of(shape)
    for dtype, bits, B, rng in configurations(shape, (name, op)):
        with precision(bits):
            what = f"backward {op} {shape} {name} {dtype.__name__} B={B}"
            boundary = ext(name, D)
            if op in ('laplace', 'laplace_axes', 'gradient'):
                a = rng.standard_normal((B,) + shape).astype(dtype)
                codes, consts = rule(name, D)
                mk = lambda ts: centred_scalar_t(ts[0], boundary, shape, backend, B)
                if op == 'laplace':
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: f.laplace(weights=0.3), lambda x, absolute: R.t_laplace(x, dx, codes, consts, [0.3] * D, absolute), what)
                elif op == 'laplace_axes':
                    w = [1.5, -0.5, 2.0][:D]
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: f.laplace(weights=tuple(w)), lambda x, absolute: R.t_laplace(x, dx, codes, consts, w, absolute), what)
                else:
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: field.spatial_gradient(f, at='center'), lambda x, absolute: R.t_gradient(x, dx, codes, consts, absolute), what)
            elif op in ('laplace_vector', 'divergence', 'curl_centred'):
                a = rng.standard_normal((B, D) + shape).astype(dtype)
                codes, consts = rule(name, D)
                mk = lambda ts: centred_vector_t(ts[0], boundary, shape, backend, B)
                if op == 'divergence':
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: f.divergence(), lambda x, absolute: R.t_divergence(x, dx, codes, consts, absolute), what)
                elif op == 'curl_centred':
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: f.curl(), lambda x, absolute: R.t_curl_centered(x, codes, consts, absolute), what)
                else:
                    fold = lambda x, absolute: R.t_laplace(x.reshape((B * D,) + shape), dx, codes, consts, [1.0] * D, absolute).reshape(x.shape)
                    _check_vjp(backend, dtype, D, [a], mk, lambda f: f.laplace(), fold, what)
            else:
                proto = StaggeredGrid(0, boundary, bounds(D), backend=backend, **res_kw(shape))
                comps = [rng.standard_normal((B,) + s).astype(dtype) for s in proto.component_shapes]
                dom = domain(name, shape)
                mk = lambda ts: StaggeredGrid(list(ts) if B > 1 else [t[0] for t in ts], boundary, bounds(D), backend=backend, **res_kw(shape))
                if op == 'curl_staggered':
                    _check_vjp(backend, dtype, D, comps, mk, lambda f: f.curl(), lambda *xs, absolute: R.t_curl_staggered(list(xs), dom, absolute), what)
                else:
                    assert op == 'laplace_staggered'
                    lap_ext = proto.boundary.spatial_gradient().spatial_gradient()
                    _check_vjp(backend, dtype, D, comps, mk, lambda f: f.laplace(), lambda *xs, absolute: R.t_laplace_staggered(list(xs), dom, 1.0, absolute), what,
                               restrict=_stored_faces_restriction(proto, lap_ext))


def centred_scalar_t(t, boundary, shape, backend, B):
    return CenteredGrid(t if B > 1 else t[0], boundary, bounds(len(shape)), backend=backend, **res_kw(shape))


def centred_vector_t(t, boundary, shape, backend, B):
    tt = torch.movedim(t, 1, -1)
    return CenteredGrid(tt if B > 1 else tt[0], boundary, bounds(len(shape)), backend=backend, **res_kw(shape))


# ---- check 5: jit_compile -------------------------------------------------------------------------------------------------------------------
def gray_scott(u, v, du, dv, f, k, dt):
    """ Reaction_Diffusion.ipynb :33-37 """
    uvv = u * v ** 2
    su = du * field.laplace(u) - uvv + f * (1 - u)
    sv = dv * field.laplace(v) + uvv - (f + k) * v
    return u + dt * su, v + dt * sv


def gray_scott_fields(size, backend, bits):
    rng = rng_for('gray-scott', size)
    dtype = np.float32 if bits == 32 else np.float64
    u = CenteredGrid((0.1 + 0.2 * rng.random((size, size))).astype(dtype), PERIODIC, x=size, y=size, backend=backend)
    v = CenteredGrid((0.1 + 0.2 * rng.random((size, size))).astype(dtype), PERIODIC, x=size, y=size, backend=backend)
    return u, v


MAZE = dict(du=0.19, dv=0.05, f=0.06, k=0.062)

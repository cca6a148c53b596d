"""
Shared cases of the method-of-lines tests (tests/test_momentum_emu.py on the emulation library, tests/test_gpu_momentum.py on the device): every check
takes the backend it runs on. References: tests/momentum_ref.py (float64), tests/diffuse_coef_ref.py.

THE FORWARD BOUND, counted from the fma chain in the header of csrc/momentum.hpp, not measured. One term W_d h_d g_d of an output carries, in units of
u = eps / 2: the difference g_d 1, the four-face mean 3, the rounded constant h_d 1, the product t_d = W_d h_d 1, a wall constant cast to T in g_d and one in
the mean 1 each -- 8 -- and at most D roundings on its way through `acc = t_x g_x; acc = fma(t_y, g_y, acc); ...`. So |out - exact| <= (8 + D) u S with
S = sum_d mean|V| (|U_hi| + |U_lo|) h_d. The float64 restatement carries (6 + D) u64 S of its own (no cast constants), which matters in the fp64 cases only:
there the constants are exact and the two add up to (6 + D) eps S; in fp32 the kernel's (4 + D / 2) eps S stands alone. K = D + 7 covers both with one eps
for the second-order terms:                      |out - ref64| <= K_FORWARD(D) eps S,   K = 9 (2-D), 10 (3-D).
THE BACKWARD BOUND, the same way. grad velocity (the longer chain): g 1 (+ 1 constant), the fma sum over the 4 (D - 1) faces + its own-component term +
the fma with 1/4: 4 (D - 1) + 1, the rounded h_d 1, h_d * acc 1, the accumulation into the output 1 -- 4 D + 2 units of u, twice that with the float64
reference's own share in the fp64 cases: (4 D + 2) eps S. grad u: G W carries 3 + 1 (+ 1 constant), the tap difference 1, h_d 1, D fmas, the accumulation 1
-- 8 + D. With one eps of slack:                 |grad - autograd64| <= K_BACKWARD(D) eps S,   K = 4 D + 3 = 11 (2-D), 15 (3-D).

THE RK4 TOLERANCES, measured on the restatement alone (tests/momentum_ref.py rk4_run, three steps of dt = 0.05, nu = 0.1, the four grids of RK4_CASES):
run A with rtol = atol = 1e-13 and a CG refresh period of 50 against run B with 1e-12 and 20. Largest deviation, relative to max|field|:
velocity 4.6e-14, pressure 1.9e-12; max|div v| after the steps: 1.9e-14. The checks allow 100 x that (the margin covers another reduction order).
"""
import os

import numpy as np
import torch

from phiflow_amd import advect, diffuse, field, fluid
from phiflow_amd.flow import PERIODIC, ZERO, ZERO_GRADIENT, Box, CenteredGrid, Solve, StaggeredGrid, combine_sides, jit_compile, l2_loss, precision, vec

import diffops_cases as DC
import diffops_ref as DR
import momentum_ref as M
from diffops_cases import (BATCHES, CENTRED_EXTS, DTYPES, SHAPES, STAGGERED_EXTS, bounds, centred_vector, centred_vector_t, domain, dx_of, eps, ext, host,
                           res_kw, rng_for, rule, staggered)

O = M.O
SMALL_SHAPES = [(2, 3), (3, 2, 4)]           # a periodic axis of 2 cells: both taps are the same sample; a closed axis of 2 cells stores one face
SMALL_EXTS = ['periodic', 'zero', 'zero_gradient']
FORWARD_CASES = [(s, n) for s in SHAPES for n in STAGGERED_EXTS] + [(s, n) for s in SMALL_SHAPES for n in SMALL_EXTS]
CENTRED_CASES = [(s, n) for s in SHAPES for n in CENTRED_EXTS] + [(s, n) for s in SMALL_SHAPES for n in SMALL_EXTS]

RK4_REL_VELOCITY = 100 * 4.6e-14
RK4_REL_PRESSURE = 100 * 1.9e-12
RK4_MAX_DIV = 100 * 1.9e-14


def K_FORWARD(D):
    return D + 7


def K_BACKWARD(D):
    return 4 * D + 3


def assert_bound(got, ref, S, K, dtype, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = K * eps(dtype) * S
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements beyond {K} eps S; worst ratio to eps S {float(np.nanmax(err / np.maximum(eps(dtype) * S, 1e-300))):.3g}"


def _faces(shape, name, B, dtype, rng):
    dom = domain(name, shape)
    return [rng.standard_normal((B,) + dom.comp_shape(d)).astype(dtype) for d in range(len(shape))]


# ---- check 2: forward, element by element -------------------------------------------------------------------------------------------------------
def check_forward_staggered(backend, shape, name):
    D = len(shape)
    dom = domain(name, shape)
    for dtype, bits in DTYPES:
        for B in BATCHES:
            rng = rng_for('momentum', shape, name, bits, B)
            with precision(bits):
                u, v, v1 = _faces(shape, name, B, dtype, rng), _faces(shape, name, B, dtype, rng), _faces(shape, name, 1, dtype, rng)
                fu, fv, fv1 = (staggered(x, ext(name, D), shape, backend) for x in (u, v, v1))
                # u != velocity; u is velocity; a batch-1 velocity shared by u's entries; a batch-1 u under a batched velocity
                for a, b, fa, fb, tag in ((u, v, fu, fv, 'u, v'), (u, u, fu, fu, 'v, v'), (u, v1, fu, fv1, 'shared velocity'), (v1, u, fv1, fu, 'shared u')):
                    out = advect.differential(fa, fb)
                    assert out.is_staggered and out.boundary == fa.boundary and out.batch_size == B
                    refs, Ss = M.advect_staggered(a, b, dom)
                    for c in range(D):
                        assert_bound(host(out.values[c]), np.broadcast_to(refs[c], out.values[c].shape), np.broadcast_to(Ss[c], out.values[c].shape), K_FORWARD(D),
                                     dtype, f"advect.differential {shape} {name} {dtype.__name__} B={B} {tag} c={c}")
                assert advect.finite_difference is advect.differential


def check_forward_centred(backend, shape, name):
    D = len(shape)
    for dtype, bits in DTYPES:
        for B in BATCHES:
            rng = rng_for('momentum centred', shape, name, bits, B)
            with precision(bits):
                u, v, v1 = (rng.standard_normal((b, D) + shape).astype(dtype) for b in (B, B, 1))
                # the velocity's extrapolation is not read: another one of the same periodicity labels the result
                v_ext = ext(name, D) if name in ('periodic', 'mixed') else ext('zero_gradient' if name != 'zero_gradient' else 'zero', D)
                fu, fv, fv1 = centred_vector(u, ext(name, D), backend), centred_vector(v, v_ext, backend), centred_vector(v1, v_ext, backend)
                for a, b, fa, fb, tag in ((u, v, fu, fv, 'u, v'), (u, u, fu, fu, 'v, v'), (u, v1, fu, fv1, 'shared velocity')):
                    out = advect.differential(fa, fb)
                    assert out.is_vector and out.boundary == fb.boundary and tuple(out.values.shape) == (B, D) + shape
                    ref, S = M.advect_centered(a, b, dx_of(shape), *rule(name, D))
                    assert_bound(host(out.values), np.broadcast_to(ref, out.values.shape), np.broadcast_to(S, out.values.shape), K_FORWARD(D), dtype,
                                 f"centred advect.differential {shape} {name} {dtype.__name__} B={B} {tag}")


def _offset_copy(t):
    """ the same values in a buffer whose first element sits one element past an aligned address """
    raw = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = raw[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def check_unaligned(backend):
    """ buffers with a storage offset of one element give the bits of aligned ones (rows that are no whole 16-byte vectors included: 7, 66 and 130 columns) """
    for shape, name in (((5, 7), 'mixed'), ((9, 66), 'lid'), ((6, 130), 'periodic'), ((3, 6, 70), 'zero_gradient'), ((2, 5, 65), 'constant')):
        D = len(shape)
        for dtype, bits in DTYPES:
            rng = rng_for('unaligned', shape, name, bits)
            with precision(bits):
                u, v = _faces(shape, name, 2, dtype, rng), _faces(shape, name, 2, dtype, rng)
                fu, fv = staggered(u, ext(name, D), shape, backend), staggered(v, ext(name, D), shape, backend)
                want = advect.differential(fu, fv)
                gu, gv = fu.with_values([_offset_copy(t) for t in fu.values]), fv.with_values([_offset_copy(t) for t in fv.values])
                got = advect.differential(gu, gv)
                for a, b in zip(want.values, got.values):
                    assert torch.equal(a, b)
                if name != 'lid':
                    cu, cv = (centred_vector(rng.standard_normal((2, D) + shape).astype(dtype), ext(name, D), backend) for _ in range(2))
                    want = advect.differential(cu, cv)
                    got = advect.differential(cu.with_values(_offset_copy(cu.values)), cv.with_values(_offset_copy(cv.values)))
                    assert torch.equal(want.values, got.values)


def check_nan_reach(backend):
    """ a NaN in one input sample reaches exactly the output samples the restatement says it reaches (no term is skipped, none is multiplied in by accident) """
    for shape, name in (((5, 7), 'periodic'), ((5, 7), 'mixed'), ((9, 8, 7), 'zero_gradient'), ((3, 6, 70), 'lid'), ((2, 3), 'periodic')):
        D = len(shape)
        dom = domain(name, shape)
        rng = rng_for('nan', shape, name)
        with precision(64):
            for which in range(2):              # the NaN sits in u / in the velocity
                for c in range(D):
                    u, v = _faces(shape, name, 1, np.float64, rng), _faces(shape, name, 1, np.float64, rng)
                    target = (u, v)[which][c]
                    spot = tuple(int(rng.integers(0, n)) for n in target.shape)
                    target[spot] = np.nan
                    out = advect.differential(staggered(u, ext(name, D), shape, backend), staggered(v, ext(name, D), shape, backend))
                    refs, _ = M.advect_staggered(u, v, dom)
                    for k in range(D):
                        assert np.array_equal(np.isnan(host(out.values[k])), np.isnan(refs[k])), (shape, name, which, c, k)
                    assert sum(int(np.isnan(r).sum()) for r in refs) > 0
            if name != 'lid':
                for which in range(2):
                    u, v = rng.standard_normal((1, D) + shape), rng.standard_normal((1, D) + shape)
                    spot = tuple(int(rng.integers(0, n)) for n in u.shape)
                    (u, v)[which][spot] = np.nan
                    out = advect.differential(centred_vector(u, ext(name, D), backend), centred_vector(v, ext(name, D), backend))
                    ref, _ = M.advect_centered(u, v, dx_of(shape), *rule(name, D))
                    assert np.array_equal(np.isnan(host(out.values)), np.isnan(ref)) and np.isnan(ref).any()


def check_marching_chunks(backend, chunk):
    """ at these shapes the launch plan gives every workgroup ONE plane: the planes per workgroup are set by hand (tuning family 0), so that the register carry
    of U's a0 neighbours runs over whole and partial chunks -- forward and both backward kernels """
    backend.ctx.set_tuning_kernel(0, 0, 0, chunk)
    try:
        for name in ('periodic', 'zero_gradient', 'constant', 'mixed', 'lid'):
            for shape in ((9, 8, 7), (3, 6, 70)):
                check_forward_staggered(backend, shape, name)
                check_backward(backend, shape, name, 'staggered')
                if name != 'lid':
                    check_forward_centred(backend, shape, name)
                    check_backward(backend, shape, name, 'centred')
    finally:
        backend.ctx.set_tuning_kernel(0, 0, 0, 0)


# ---- check 3: hand values ---------------------------------------------------------------------------------------------------------------------------
def check_hand_values(backend):
    with precision(64):
        b = Box(x=(0.3, 2.1), y=(-1.0, 1.5))
        # rigid rotation v = (-y, x): -(v . grad) v = (x, y); linear fields make the differences and the four-face means exact
        vs = StaggeredGrid(lambda x, y: (-y, x), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        want = StaggeredGrid(lambda x, y: (x, y), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        out = advect.differential(vs, vs)
        for got, w in zip(out.numpy(), want.numpy()):
            np.testing.assert_allclose(got[1:-1, 1:-1], w[1:-1, 1:-1], rtol=0, atol=1e-12)
        vc = CenteredGrid(lambda x, y: vec(x=-y, y=x), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        wc = CenteredGrid(lambda x, y: vec(x=x, y=y), ZERO_GRADIENT, b, x=6, y=5, backend=backend)
        np.testing.assert_allclose(advect.differential(vc, vc).numpy()[1:-1, 1:-1], wc.numpy()[1:-1, 1:-1], rtol=0, atol=1e-12)
        # a uniform velocity U e_x over sin(k x): -U (sin k (x + dx) - sin k (x - dx)) / (2 dx)
        n, U, k = 16, 0.7, 3.0
        pb = Box(x=(0.0, 2 * np.pi), y=(0.0, 1.0))
        dx = 2 * np.pi / n
        vel = StaggeredGrid((U, 0.0), PERIODIC, pb, x=n, y=4, backend=backend)
        u = StaggeredGrid(lambda x, y: (np.sin(k * x), 0 * x), PERIODIC, pb, x=n, y=4, backend=backend)
        got = advect.differential(u, vel).numpy()
        xf = np.arange(n)[:, None] * dx + 0 * np.arange(4)[None, :]
        np.testing.assert_allclose(got[0], -U * (np.sin(k * (xf + dx)) - np.sin(k * (xf - dx))) / (2 * dx), rtol=0, atol=1e-13)
        np.testing.assert_array_equal(got[1], 0 * got[1])
        velc = CenteredGrid((U, 0.0), PERIODIC, pb, x=n, y=4, backend=backend)
        uc = CenteredGrid(lambda x, y: vec(x=np.sin(k * x), y=0 * x), PERIODIC, pb, x=n, y=4, backend=backend)
        xc = xf + 0.5 * dx
        np.testing.assert_allclose(advect.differential(uc, velc).numpy()[..., 0], -U * (np.sin(k * (xc + dx)) - np.sin(k * (xc - dx))) / (2 * dx), rtol=0, atol=1e-13)


def check_storage_facts(backend):
    """ the result's kind, boundary and shapes: a staggered result is `u.with_values` (advect.py:116), a centred one `velocity.with_values` (:124) """
    b = Box(x=(0.3, 2.1), y=(-1.0, 1.5))
    for name in STAGGERED_EXTS:
        u = StaggeredGrid(0.5, ext(name, 2), b, x=5, y=7, backend=backend)
        out = advect.differential(u, u)
        assert out.is_staggered and out.boundary == u.boundary and [tuple(t.shape) for t in out.values] == [tuple(t.shape) for t in u.values]
        assert out.bounds is u.bounds and out.resolution == u.resolution
    for name in CENTRED_EXTS:
        u = CenteredGrid((1.0, 2.0), ext(name, 2), b, x=5, y=7, backend=backend)
        vel = CenteredGrid((0.5, -1.0), PERIODIC if name == 'periodic' else (combine_sides(x=PERIODIC, y=ZERO_GRADIENT) if name == 'mixed' else ZERO_GRADIENT),
                           b, x=5, y=7, backend=backend)
        out = advect.differential(u, vel)
        assert out.is_vector and out.boundary == vel.boundary and tuple(out.values.shape) == (1, 2, 5, 7)
    p = CenteredGrid(1.0, ZERO_GRADIENT, b, x=5, y=7, backend=backend)
    assert p.sampled_at == 'center' and StaggeredGrid(0, 0, b, x=5, y=7, backend=backend).sampled_at == 'face'
    g = p.gradient(at='face')
    assert g.is_staggered and g.boundary == ZERO and p.gradient().is_vector         # the method's default location is 'center'


# ---- check 4: backward ----------------------------------------------------------------------------------------------------------------------------
def check_backward(backend, shape, name, kind):
    """ every sample of both gradients against torch autograd of the float64 restatement, |grad - ref| <= K_BACKWARD eps S, S = the autograd of the absolute
    restatement against |grad_out|; u != velocity and u is velocity (the sum of the two gradients) """
    D = len(shape)
    dom = domain(name, shape) if kind == 'staggered' else None
    for dtype, bits in DTYPES:
        for B in BATCHES:
            rng = rng_for('momentum backward', shape, name, kind, bits, B)
            tdt = torch.float32 if dtype == np.float32 else torch.float64
            with precision(bits):
                if kind == 'staggered':
                    u, v = _faces(shape, name, B, dtype, rng), _faces(shape, name, B, dtype, rng)
                    mk = lambda ts: StaggeredGrid(list(ts) if B > 1 else [t[0] for t in ts], ext(name, D), bounds(D), backend=backend, **res_kw(shape))
                    fn = lambda xs, ys, absolute: M.t_advect_staggered(list(xs), list(ys), dom, absolute)
                    split = lambda xs: (xs[:D], xs[D:])
                    values = lambda f: list(f.values)
                else:
                    u, v = [rng.standard_normal((B, D) + shape).astype(dtype)], [rng.standard_normal((B, D) + shape).astype(dtype)]
                    mk = lambda ts: centred_vector_t(ts[0], ext(name, D), shape, backend, B)
                    fn = lambda xs, ys, absolute: [M.t_advect_centered(xs[0], ys[0], dx_of(shape), *rule(name, D), absolute)]
                    split = lambda xs: (xs[:1], xs[1:])
                    values = lambda f: [f.values]
                for same in (False, True):
                    arrays = u if same else u + v
                    leaves = [torch.tensor(a, dtype=tdt, device=backend.device, requires_grad=True) for a in arrays]
                    fu = mk(leaves[:len(u)])
                    out = advect.differential(fu, fu if same else mk(leaves[len(u):]))
                    outs = values(out)
                    gouts = [rng.standard_normal(tuple(o.shape)).astype(dtype) for o in outs]
                    torch.autograd.backward(outs, [torch.tensor(g, device=backend.device) for g in gouts])
                    rest = (lambda *xs, absolute: fn(xs, xs, absolute)) if same else (lambda *xs, absolute: fn(*split(xs), absolute))
                    ref = DR.vjp(lambda *xs: rest(*xs, absolute=False), arrays, gouts)
                    # (the absolute restatement at |inputs|: the operator is bilinear, its absolute form differentiates to sum |G| |W| h at non-negative inputs)
                    S = DR.vjp(lambda *xs: rest(*xs, absolute=True), [np.abs(a) for a in arrays], [np.abs(g) for g in gouts])
                    for k, (t, r, s) in enumerate(zip(leaves, ref, S)):
                        assert_bound(host(t.grad), r, s, K_BACKWARD(D), dtype, f"backward {kind} {shape} {name} {dtype.__name__} B={B} same={same} input {k}")


def check_backward_accumulates(backend):
    """ the *_backward entries add to their outputs: two calls into zeroed buffers give exactly twice one call (x + x is exact) """
    from phiflow_amd.field import _cell_grid
    rng = rng_for('momentum accumulate')
    shape = (5, 66)
    c = backend.ctx
    P = lambda ts: [t.data_ptr() for t in ts]
    with precision(32):
        u, v, g = (staggered(_faces(shape, 'mixed', 2, np.float32, rng), ext('mixed', 2), shape, backend) for _ in range(3))
        cu, cv, cg = (centred_vector(rng.standard_normal((2, 2) + shape).astype(np.float32), ext('mixed', 2), backend) for _ in range(3))
        codes, consts = rule('mixed', 2)
        grid, cgrid = u.grid_struct(), _cell_grid(cu)
        zeros_s = lambda: [torch.zeros_like(t) for t in u.values]
        zeros_c = lambda: [torch.zeros_like(cu.values)]
        calls = [
            (lambda o: c.advect_differential_backward(grid, P(u.values), P(v.values), P(g.values), P(o), None, backend.stream()), zeros_s),
            (lambda o: c.advect_differential_backward(grid, P(u.values), P(v.values), P(g.values), None, P(o), backend.stream()), zeros_s),
            (lambda o: c.advect_differential_centered_backward(cgrid, cu.values.data_ptr(), codes, consts, cv.values.data_ptr(), cg.values.data_ptr(),
                                                               o[0].data_ptr(), 0, backend.stream()), zeros_c),
            (lambda o: c.advect_differential_centered_backward(cgrid, cu.values.data_ptr(), codes, consts, cv.values.data_ptr(), cg.values.data_ptr(),
                                                               0, o[0].data_ptr(), backend.stream()), zeros_c),
        ]
        for call, zeros in calls:
            once, twice = zeros(), zeros()
            call(once)
            call(twice)
            call(twice)
            for a1, a2 in zip(once, twice):
                assert float(a1.abs().max()) > 0 and torch.equal(a2, 2 * a1)


# ---- check 5: diffuse.differential ------------------------------------------------------------------------------------------------------------------
def check_diffuse_differential(backend):
    import diffuse_coef_ref as CR
    assert diffuse.finite_difference is diffuse.differential
    rng = rng_for('diffuse.differential')
    expect = {'periodic': PERIODIC, 'zero_gradient': ZERO_GRADIENT, 'zero': ZERO, 'constant': ZERO, 'mixed': None, 'lid': ZERO}
    for bits, dtype in ((32, np.float32), (64, np.float64)):
        with precision(bits):
            for shape in ((5, 7), (3, 6, 7)):
                D = len(shape)
                for name in STAGGERED_EXTS:
                    v = staggered(_faces(shape, name, 2, dtype, rng), ext(name, D), shape, backend)
                    out = diffuse.differential(v, 0.3)
                    lap = field.laplace(v, weights=0.3)
                    # values: the bits of laplace(u, weights=k) on the faces laplace keeps (it re-stores BOUNDARY -> ZERO); the layout stays u's
                    assert out.is_staggered and [tuple(t.shape) for t in out.values] == [tuple(t.shape) for t in v.values]
                    for a, b in zip(v.with_values(list(out.values)).with_boundary(lap.boundary).values, lap.values):
                        assert torch.equal(a, b)
                    if expect[name] is not None:
                        assert out.boundary == expect[name], (name, out.boundary)
                    else:
                        sides = [out.boundary.side(d, up) for d in 'xyz'[:D] for up in (False, True)]
                        assert sides[:2] == [PERIODIC, PERIODIC] and sides[2:4] == [ZERO, ZERO_GRADIENT]
                for name in CENTRED_EXTS:
                    for u in (DC.centred_scalar(rng.standard_normal((2,) + shape).astype(dtype), ext(name, D), backend),
                              centred_vector(rng.standard_normal((2, D) + shape).astype(dtype), ext(name, D), backend)):
                        per_axis = tuple([1.5, -0.5, 2.0][:D])
                        for k in (0.3, per_axis, vec(**dict(zip('xyz', per_axis)))):
                            out = diffuse.differential(u, k)
                            assert torch.equal(out.values, field.laplace(u, weights=k).values) and out.is_vector == u.is_vector
                            if expect[name] is not None:
                                assert out.boundary == expect[name]
    # a Field diffusivity: the flux form of diffuse.py:129-136 against tests/diffuse_coef_ref.py. out = (u + L u) - u: the stencil's roundings and one of |u + L u|,
    # bounded by 16 eps times the sum of the absolute weights of I + L times max|u|
    with precision(64):
        shape = (9, 8)
        for name in CENTRED_EXTS:
            a = rng.standard_normal((2,) + shape)
            kf = 0.5 + rng.random((1,) + shape)
            u = DC.centred_scalar(a, ext(name, 2), backend)
            coef = DC.centred_scalar(kf, ZERO_GRADIENT if name != 'periodic' else PERIODIC, backend)
            out = diffuse.differential(u, coef)
            codes, consts = rule(name, 2)
            ccodes = [[O.PERIODIC if c == O.PERIODIC else O.OPEN for c in pair] for pair in codes]
            w = [1.0 / (h * h) for h in dx_of(shape)]
            ref = CR.lap(a, kf, w, codes, consts, ccodes, [(0.0, 0.0)] * 2)
            scale = np.abs(a).max() * (1 + sum(4 * kf.max() * x for x in w))         # the sum of the absolute stencil weights of I + L
            assert np.abs(host(out.values) - ref).max() <= 16 * eps(np.float64) * scale, name
            assert not out.is_staggered and out.boundary == (expect[name] if expect[name] is not None else out.boundary)
        # the backward runs (w.r.t. u, wherever laplace is differentiable)
        for make in (lambda t: CenteredGrid(t, 0.7, bounds(2), backend=backend, **res_kw(shape)),
                     lambda t: StaggeredGrid([t, 2 * t], PERIODIC, bounds(2), backend=backend, **res_kw(shape))):
            t = torch.tensor(rng.standard_normal(shape), device=backend.device, requires_grad=True)
            out = diffuse.differential(make(t), 0.3)
            l2_loss(out).backward()
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


# ---- check 6: incompressible_rk4 ------------------------------------------------------------------------------------------------------------------
_P, _C = O.PERIODIC, O.CLOSED
RK4_CASES = {
    'periodic 16x12': ((16, 12), [(_P, _P), (_P, _P)]),
    'closed 12x16': ((12, 16), [(_C, _C), (_C, _C)]),
    'mixed 16x12': ((16, 12), [(_P, _P), (_C, _C)]),
    'periodic 6x8x10': ((6, 8, 10), [(_P, _P)] * 3),
}
RK4_SIZES = [2 * np.pi, 1.7 * np.pi, 2.2 * np.pi]
RK4_DT, RK4_NU = 0.05, 0.1
_RK4_REFERENCE = {}


def pde(v, nu):
    return advect.differential(v, v) + diffuse.differential(v, nu)


def rk4_setup(case):
    """ (domain, velocity arrays, pressure array, velocity extrapolation, pressure extrapolation, Box) of a case: a projected random field """
    shape, bc = RK4_CASES[case]
    D = len(shape)
    dom = O.Domain(shape, (0.0,) * D, tuple(RK4_SIZES[:D]), tuple(bc))
    rng = rng_for('rk4', case)
    v0 = [0.5 * rng.standard_normal((1,) + dom.comp_shape(d)) for d in range(D)]
    v0, _, _, _ = O.make_incompressible(v0, dom, rtol=1e-13, atol=1e-13, max_iter=4000)
    sides = {d: (PERIODIC if lo == _P else 0) for d, (lo, _) in zip('xyz', bc)}
    p_sides = {d: (PERIODIC if lo == _P else ZERO_GRADIENT) for d, (lo, _) in zip('xyz', bc)}
    box = Box(**{d: (0.0, s) for d, s in zip('xyz'[:D], RK4_SIZES)})
    return dom, v0, np.zeros((1,) + shape), combine_sides(**sides), combine_sides(**p_sides), box


def rk4_reference(case):
    """ the restatement after 1 and after 3 steps, computed once per process and left unchanged """
    if case not in _RK4_REFERENCE:
        dom, v0, p0, _, _, _ = rk4_setup(case)
        v1, p1 = M.rk4_step(v0, p0, RK4_DT, RK4_NU, dom)
        v3, p3 = M.rk4_run(v1, p1, RK4_DT, 2, RK4_NU, dom)
        _RK4_REFERENCE[case] = {1: (v1, p1), 3: (v3, p3)}
    return _RK4_REFERENCE[case]


def check_rk4_reference_spread():
    """ the measurement behind RK4_REL_*: two runs of the restatement alone (tolerance 1e-13 / refresh 50 against 1e-12 / refresh 20) stay inside 1 / 100 of
    the tolerances the device checks use """
    for case in RK4_CASES:
        dom, v0, p0, _, _, _ = rk4_setup(case)
        va, pa = rk4_reference(case)[3]
        vb, pb = M.rk4_run(v0, p0, RK4_DT, 3, RK4_NU, dom, rtol=1e-12, atol=1e-12, refresh=20)
        dev_v = max(np.abs(a - b).max() for a, b in zip(va, vb)) / max(np.abs(a).max() for a in va)
        dev_p = np.abs(pa - pb).max() / np.abs(pa).max()
        div = np.abs(O.divergence(va, dom)).max()
        print(f"rk4 restatement spread {case}: velocity {dev_v:.3g} pressure {dev_p:.3g} max|div| {div:.3g}")
        assert dev_v <= RK4_REL_VELOCITY / 100 and dev_p <= RK4_REL_PRESSURE / 100 and div <= RK4_MAX_DIV / 100


def check_rk4(backend, case):
    dom, v0, p0, v_ext, p_ext, box = rk4_setup(case)
    shape = RK4_CASES[case][0]
    with precision(64):
        v = StaggeredGrid([a[0] for a in v0], v_ext, box, backend=backend, **res_kw(shape))
        p = CenteredGrid(0, p_ext, box, backend=backend, **res_kw(shape))
        solve = Solve('CG', 1e-13, 1e-13, max_iterations=4000)
        for step in (1, 2, 3):
            v, p = fluid.incompressible_rk4(pde, v, p, RK4_DT, pressure_order=2, pressure_solve=solve, nu=RK4_NU)
            assert v.is_staggered and v.boundary == v_ext and p.is_centered and [tuple(t.shape[1:]) for t in v.values] == [dom.comp_shape(d) for d in range(len(shape))]
            if step in (1, 3):
                rv, rp = rk4_reference(case)[step]
                ev = max(np.abs(host(a) - b).max() for a, b in zip(v.values, rv)) / max(np.abs(b).max() for b in rv)
                ep = np.abs(host(p.values) - rp).max() / np.abs(rp).max()
                div = float(field.divergence(v).values.abs().max())
                print(f"rk4 {case} step {step}: velocity {ev:.3g} pressure {ep:.3g} max|div| {div:.3g}")
                assert ev <= RK4_REL_VELOCITY and ep <= RK4_REL_PRESSURE and div <= RK4_MAX_DIV, (case, step, ev, ep, div)


def _tg_fields(n, backend, perturbed=False):
    dom = M.periodic_domain((n, n))
    v0 = M.taylor_green(dom, perturbed)
    box = Box(x=(0.0, 2 * np.pi), y=(0.0, 2 * np.pi))
    v = StaggeredGrid([a[0] for a in v0], PERIODIC, box, x=n, y=n, backend=backend)
    return dom, v0, v, CenteredGrid(0, PERIODIC, box, x=n, y=n, backend=backend)


def _run(v, p, dt, steps, nu, solve):
    for _ in range(steps):
        v, p = fluid.incompressible_rk4(pde, v, p, dt, pressure_order=2, pressure_solve=solve, nu=nu)
    return v, p


ENERGY_FACTS = {16: 0.0041, 32: 0.00103}         # relative error of E(0.8) / E(0) against exp(-4 nu T), nu = 0.1, dt = 0.1: the restatement's figures


def energy_error(run, n):
    """ run(v0 arrays, p0, dt, steps) -> velocity arrays """
    dom = M.periodic_domain((n, n))
    v0 = M.taylor_green(dom)
    v = run(n, 0.1, 8)
    return M.energy(v) / M.energy(v0) / np.exp(-4 * 0.1 * 0.8) - 1


def order_ratios(run):
    """ error ratios on halving dt, 0.1 -> 0.05 -> 0.025 against a dt = 0.00625 run (16^2, perturbed field, T = 0.4): run(dt, steps) -> velocity arrays """
    ref = run(0.00625, 64)
    errs = [max(np.abs(a - b).max() for a, b in zip(run(dt, int(round(0.4 / dt))), ref)) for dt in (0.1, 0.05, 0.025)]
    return errs[0] / errs[1], errs[1] / errs[2]


def check_rk4_accuracy(backend):
    """ the two facts of the restatement, on the device: the energy error of the Taylor-Green decay and the temporal order """
    with precision(64):
        solve = Solve('CG', 1e-13, 1e-13, max_iterations=4000)

        def tg(n, dt, steps):
            _, _, v, p = _tg_fields(n, backend)
            return [host(t) for t in _run(v, p, dt, steps, 0.1, solve)[0].values]
        for n, fact in ENERGY_FACTS.items():
            err = energy_error(tg, n)
            print(f"energy error {n}^2: {err:.4%}")
            assert abs(err) <= 1.25 * fact, (n, err)

        def perturbed(dt, steps):
            _, _, v, p = _tg_fields(16, backend, True)
            return [host(t) for t in _run(v, p, dt, steps, 0.1, solve)[0].values]
        r1, r2 = order_ratios(perturbed)
        print(f"error ratios on halving dt: {r1:.3g} {r2:.3g}")
        assert r1 >= 6 and r2 >= 6, (r1, r2)


def check_rk4_fp32(backend):
    """ one periodic case in float32 with the solve tolerance 1e-5, under the convention of tests/golden_cases.py `_close`: max error relative to max|reference|,
    2e-4 as for the fp32 velocities and pressures of the golden runs there (solves of 1e-5, a few steps) """
    from golden_cases import _close
    case = 'periodic 16x12'
    dom, v0, p0, v_ext, p_ext, box = rk4_setup(case)
    shape = RK4_CASES[case][0]
    with precision(32):
        v = StaggeredGrid([a[0].astype(np.float32) for a in v0], v_ext, box, backend=backend, **res_kw(shape))
        p = CenteredGrid(0, p_ext, box, backend=backend, **res_kw(shape))
        v, p = _run(v, p, RK4_DT, 3, RK4_NU, Solve('CG', 1e-5, 0))
        assert v.dtype == torch.float32
        rv, rp = rk4_reference(case)[3]
        for c, (a, b) in enumerate(zip(v.values, rv)):
            _close(host(a), b, 2e-4, f"velocity component {c}")
        _close(host(p.values), rp, 2e-4, "pressure")


def check_rk4_jit(backend):
    """ a jit_compile'd RK4 step replays the eager bits over the capture and three replays (32^2, fp32) """
    with precision(32):
        _, _, v0, p0 = _tg_fields(32, backend, True)
        solve = Solve('CG', 1e-5, 0, max_iterations=200)
        eager = lambda v, p: fluid.incompressible_rk4(pde, v, p, 0.05, pressure_order=2, pressure_solve=solve, nu=0.1)
        step = jit_compile(eager)
        ve, pe, vj, pj = v0, p0, v0, p0
        for _ in range(4):
            ve, pe = eager(ve, pe)
            vj, pj = step(vj, pj)
            for a, b in zip(ve.numpy() + [pe.numpy()], vj.numpy() + [pj.numpy()]):
                assert np.array_equal(a, b)
        assert float(np.abs(ve.numpy()[0]).max()) > 0.1


def check_rk4_gradient(backend):
    """ the gradient of l2_loss through one RK4 step w.r.t. the velocity is finite and matches a central finite difference of the loss (fp64, 8 x 8), for three
    perturbation directions. The difference quotient with h = 1e-5 carries h^2 |f'''| ~ 1e-10 and eps |loss| / h ~ 1e-10 of the loss: 1e-6 relative to the
    directional derivative's scale sum|grad| |direction| is five digits above both. """
    with precision(64):
        n = 8
        dom, v0, _, p = _tg_fields(n, backend, True)
        box = Box(x=(0.0, 2 * np.pi), y=(0.0, 2 * np.pi))
        solve = Solve('CG', 1e-13, 1e-13, max_iterations=2000)

        def loss_of(arrays, grad=False):
            ts = [torch.tensor(a[0], device=backend.device, requires_grad=grad) for a in arrays]
            v = StaggeredGrid(ts, PERIODIC, box, x=n, y=n, backend=backend)
            v1, _ = fluid.incompressible_rk4(pde, v, p, 0.1, pressure_order=2, pressure_solve=solve, nu=0.1)
            return l2_loss(v1), ts
        loss, leaves = loss_of(v0, True)
        loss.backward()
        grads = [host(t.grad) for t in leaves]
        assert all(np.isfinite(g).all() for g in grads) and max(np.abs(g).max() for g in grads) > 0
        rng = rng_for('rk4 gradient')
        h = 1e-5
        for _ in range(3):
            direction = [rng.standard_normal(a.shape) for a in v0]
            plus = float(loss_of([a + h * d for a, d in zip(v0, direction)])[0])
            minus = float(loss_of([a - h * d for a, d in zip(v0, direction)])[0])
            fd = (plus - minus) / (2 * h)
            an = sum(float((g * d[0]).sum()) for g, d in zip(grads, direction))
            scale = sum(float((np.abs(g) * np.abs(d[0])).sum()) for g, d in zip(grads, direction))
            print(f"rk4 gradient: analytic {an:.10g} finite difference {fd:.10g}")
            assert abs(an - fd) <= 1e-6 * scale, (an, fd, scale)


# ---- check 7: refusals ------------------------------------------------------------------------------------------------------------------------------
def refusal_cases(backend):
    """ (label, call, a word the message must hold: the way out) """
    b = Box(x=(0.0, 1.0), y=(0.0, 1.0))
    st = StaggeredGrid(0.5, 0, b, x=5, y=7, backend=backend)
    st_open = StaggeredGrid(0.5, ZERO_GRADIENT, b, x=5, y=7, backend=backend)
    st_other = StaggeredGrid(0.5, 0, b, x=6, y=7, backend=backend)
    st_lid = StaggeredGrid(0.5, {'x': 0, 'y-': 0, 'y+': vec(x=1, y=0)}, b, x=5, y=7, backend=backend)
    cv = CenteredGrid((1.0, 2.0), ZERO_GRADIENT, b, x=5, y=7, backend=backend)
    cv_vec = CenteredGrid((1.0, 2.0), {'x': 0, 'y-': 0, 'y+': vec(x=1, y=0)}, b, x=5, y=7, backend=backend)
    cs = CenteredGrid(1.0, ZERO_GRADIENT, b, x=5, y=7, backend=backend)
    s1 = StaggeredGrid(0.5, 0, Box(x=(0.0, 1.0)), x=5, backend=backend)
    p = CenteredGrid(0, ZERO_GRADIENT, b, x=5, y=7, backend=backend)
    rk4 = lambda v, q=p, **kw: fluid.incompressible_rk4(lambda w, **_: advect.differential(w, w), v, q, 0.1, **kw)
    return [
        ('order', lambda: advect.differential(st, st, order=4), 'order=2'),
        ('implicit', lambda: advect.differential(st, st, implicit=Solve('CG')), 'implicit=None'),
        ('centred scalar u', lambda: advect.differential(cs, cv), 'vector'),
        ('kinds', lambda: advect.differential(st, cv), '@'),
        ('kinds 2', lambda: advect.differential(cv, st), '@'),
        ('scalar velocity', lambda: advect.differential(cv, cs), 'vector'),
        ('grids', lambda: advect.differential(st, st_other), '@'),
        ('boundary', lambda: advect.differential(st_open, st), 'with_boundary'),
        ('vector constant', lambda: advect.differential(cv_vec, cv), 'number'),
        ('1-D', lambda: advect.differential(s1, s1), '2-D'),
        ('diffuse order', lambda: diffuse.differential(st, 0.1, order=4), 'order=2'),
        ('diffuse staggered Field', lambda: diffuse.differential(st, cs), 'CenteredGrid'),
        ('diffuse staggered per-axis', lambda: diffuse.differential(st, (1.0, 2.0)), 'CenteredGrid'),
        ('diffuse implicit', lambda: diffuse.differential(cs, 0.1, implicit=Solve('CG')), 'implicit=None'),
        ('rk4 default pressure order', lambda: rk4(st), 'pressure_order=2'),
        ('rk4 pressure order 6', lambda: rk4(st, pressure_order=6), 'pressure_order=2'),
        ('rk4 non-zero constant', lambda: rk4(st_lid, pressure_order=2), 'zero walls'),
        ('rk4 open', lambda: rk4(st_open, pressure_order=2), 'PERIODIC'),
        ('rk4 centred', lambda: rk4(cv, pressure_order=2), 'StaggeredGrid'),
        ('rk4 obstacles', lambda: rk4(st, pressure_order=2, obstacles=[Box(x=(0.2, 0.4), y=(0.2, 0.4))]), 'make_incompressible'),
    ]

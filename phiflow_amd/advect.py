"""
Advection schemes backed by libphihip (reference: phi/physics/advect.py).
Implemented on the HIP backend: `semi_lagrangian` / `advect` / `mac_cormack` with the `euler` (fused kernels) and `rk4` / `finite_rk4` integrators for StaggeredGrid
and CenteredGrid fields advected by a StaggeredGrid velocity, and for centred scalar / vector fields advected by a centred vector velocity (Burgers'
equation: `advect.semi_lagrangian(v, v, dt)` of a CenteredGrid), and `differential` / `finite_difference`, the central-difference term -(v . grad) u
of a method-of-lines step. Anything else raises `NotImplementedError`.
"""
from typing import Callable

import torch

from . import autodiff
from .extrapolation import ConstantExtrapolation, resolve
from .field import Field, _ptrs


def euler(data: Field, velocity: Field, dt: float, v0=None):
    """ Euler integrator marker (phi/physics/advect.py:20-24). The back-trace itself is fused into the HIP kernel, so this
    function only identifies the integrator when passed to `semi_lagrangian`. """
    raise NotImplementedError("euler() is fused into the HIP semi-Lagrangian kernel; pass it as `integrator=euler`")


def rk4(data: Field, velocity: Field, dt: float, v0=None):
    """ Runge-Kutta-4 integrator marker (phi/physics/advect.py:27-36): `semi_lagrangian(..., integrator=rk4)` traces the sample points
    back with four velocity evaluations (sampling.integrate_points) instead of one. """
    raise NotImplementedError("pass rk4 as `integrator=rk4`")


def finite_rk4(data: Field, velocity: Field, dt: float, v0=None):
    """ rk4 with Euler fallback where the velocity is not finite (phi/physics/advect.py:38-47); marker like `rk4` """
    raise NotImplementedError("pass finite_rk4 as `integrator=finite_rk4`")


def semi_lagrangian(field: Field, velocity: Field, dt: float, integrator: Callable = euler) -> Field:
    """ Semi-Lagrangian advection with backward Euler lookup (phi/physics/advect.py:156-179).

    Args:
        field: quantity to be advected (`StaggeredGrid` or `CenteredGrid`)
        velocity: `StaggeredGrid`, or a centred vector `CenteredGrid` for a centred field; on the same grid the fused kernels run, otherwise
            the general sampling path (sampling.py)
        dt: time increment
        integrator: `euler` (fused kernels), `rk4` or `finite_rk4` (general sampling path)

    Returns:
        Field with the same sample points and boundary as `field`
    """
    return _advect(field, velocity, dt, integrator, None)


def _scalar_boundary(field: Field):
    s_codes, s_vals = resolve(field.boundary, field.dims)
    s_val = [[s_vals[a][s][0] if isinstance(field.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)]
             for a, d in enumerate(field.dims)]
    return s_codes, s_val


def _advect(field: Field, velocity: Field, dt: float, integrator: Callable, correction_strength) -> Field:
    """ shared argument handling of semi_lagrangian (correction_strength None) and mac_cormack """
    from .field import require_plain
    require_plain(field, 'advect'); require_plain(velocity, 'advect (velocity)')
    if integrator not in (euler, rk4, finite_rk4):
        raise NotImplementedError("HIP backend: grid advection supports the integrators euler, rk4 and finite_rk4")
    from . import sampling
    if velocity.is_centered:
        return _advect_by_centered(field, velocity, dt, integrator, correction_strength)
    if field.is_vector:     # a centred vector field by a staggered velocity: gathers at explicit coordinates
        return sampling.advect_general(field, velocity, float(dt), correction_strength, integrator.__name__)
    if integrator is not euler:   # Runge-Kutta back-trace: explicit velocity evaluations at the intermediate points
        return sampling.advect_general(field, velocity, float(dt), correction_strength, integrator.__name__)
    if not sampling.same_grid(field, velocity):
        # "velocity need not be sampled at same locations as field" (advect.py:193): gathers at explicit coordinates instead of the
        # fused kernels (Batched_Smoke.ipynb: 200^2 smoke advected by a 64^2 velocity)
        return sampling.advect_general(field, velocity, float(dt), correction_strength)
    be = velocity.backend
    assert field.dtype == velocity.dtype, "field and velocity must have the same precision"
    B = max(field.batch_size, velocity.batch_size)
    vel = [_expand(t, B) for t in velocity.values]
    grid = velocity.grid_struct(batch=B)
    if field.is_staggered:
        same_layout = [tuple(a.shape[1:]) for a in field.values] == [tuple(b.shape[1:]) for b in velocity.values]
        if not same_layout or resolve(field.boundary, field.dims) != resolve(velocity.boundary, velocity.dims):
            raise NotImplementedError("HIP backend: an advected StaggeredGrid must share the velocity's boundary conditions")
        src = vel if field is velocity else [_expand(t, B) for t in field.values]
        if autodiff.needs_grad(*src, *vel):
            if correction_strength is not None:
                out = list(autodiff.MacCormackStaggered.apply(dict(be=be, grid=grid, dt=float(dt), strength=correction_strength), *src, *vel))
            else:
                out = list(autodiff.SemiLagrangianStaggered.apply(dict(be=be, grid=grid, dt=float(dt)), *src, *vel))
            return Field(field.resolution, field.bounds, field.boundary, out, True, be, field.batched or velocity.batched)
        out = [torch.empty_like(t) for t in src]
        if correction_strength is None:
            be.ctx.advect_staggered(grid, _ptrs(src), _ptrs(vel), _ptrs(out), dt, be.stream())
        else:
            be.ctx.mac_cormack_staggered(grid, _ptrs(src), _ptrs(vel), _ptrs(out), dt, correction_strength, be.stream())
        return Field(field.resolution, field.bounds, field.boundary, out, True, be, field.batched or velocity.batched)
    src = _expand(field.values, B)
    s_codes, s_val = _scalar_boundary(field)
    if autodiff.needs_grad(src, *vel):
        meta = dict(be=be, grid=grid, dt=float(dt), s_codes=s_codes, s_val=s_val, strength=correction_strength)
        fn = autodiff.SemiLagrangianCentered if correction_strength is None else autodiff.MacCormackCentered
        return Field(field.resolution, field.bounds, field.boundary, fn.apply(meta, src, *vel), False, be, field.batched or velocity.batched)
    out = torch.empty_like(src)
    if correction_strength is None:
        be.ctx.advect_centered(grid, src.data_ptr(), s_codes, s_val, _ptrs(vel), out.data_ptr(), dt, be.stream())
    else:
        be.ctx.mac_cormack_centered(grid, src.data_ptr(), s_codes, s_val, _ptrs(vel), out.data_ptr(), dt, correction_strength, be.stream())
    return Field(field.resolution, field.bounds, field.boundary, out, False, be, field.batched or velocity.batched)


def _advect_by_centered(field: Field, velocity: Field, dt: float, integrator: Callable, correction_strength) -> Field:
    """ a centred scalar or vector field advected by a centred vector velocity. euler, same grid, no gradient: one launch of
    `phihip_advect_centered_vector` (the velocity at the cell is the stored value, the taps are shared by the components); everything else
    through the general sampling path, which differentiates through GridSample. """
    from . import sampling
    from .field import _centered_rule, _torch_dtype_code
    from . import _capi
    if field.is_staggered:
        raise NotImplementedError("HIP backend: advecting a StaggeredGrid by a centred velocity is not implemented; pass the StaggeredGrid "
                                  "velocity (`StaggeredGrid(v, ...)`) or advect a CenteredGrid")
    if not velocity.is_vector:
        raise NotImplementedError("HIP backend: the advecting velocity is a centred SCALAR field; pass a vector field (StaggeredGrid or a "
                                  "CenteredGrid with a vector axis)")
    assert field.dtype == velocity.dtype, "field and velocity must have the same precision"
    fused = integrator is euler and correction_strength is None and sampling.same_grid(field, velocity) \
        and not autodiff.needs_grad(field.values, velocity.values)
    if not fused:
        return sampling.advect_general(field, velocity, float(dt), correction_strength, integrator.__name__)
    be = field.backend
    s_codes, s_val = _centered_rule(field, 'advect')
    B = max(field.batch_size, velocity.batch_size)
    D = field.spatial_rank
    C = D if field.is_vector else 1
    src = field.values.contiguous()
    vel = src if field is velocity else velocity.values.contiguous()
    grid = _capi.make_grid(D, _torch_dtype_code(field.dtype), B, list(field.resolution.values()), field.bounds.lower, field.bounds.upper, s_codes)
    out = torch.empty((B,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    be.ctx.advect_centered_vector(grid, src.data_ptr(), src.shape[0], C, s_codes, s_val, vel.data_ptr(), vel.shape[0], out.data_ptr(), dt, be.stream())
    return Field(field.resolution, field.bounds, field.boundary, out, False, be, field.batched or velocity.batched, vector=field.is_vector)


def advect(field: Field, velocity: Field, dt: float, integrator: Callable = euler) -> Field:
    """ `advect.advect` for grids == `semi_lagrangian` (phi/physics/advect.py:50-75) """
    return semi_lagrangian(field, velocity, dt, integrator=integrator)


def differential(u: Field, velocity: Field, density: float = 1., order=2, implicit=None, upwind=True) -> Field:
    """ The differential advection term -(velocity . grad) u as it stands on the right-hand side of a PDE, with central differences
    (phi/physics/advect.py:78-133, grid branches :108-124; csrc/momentum.hpp). `density` and `upwind` are accepted and, as in the
    reference's grid branches, not read.

    StaggeredGrid `u` with a StaggeredGrid `velocity` on the same grid and boundary (`u` may be the velocity itself): for component c at its stored face f
    `-sum_d W_d(f) (U_c[f + e_d] - U_c[f - e_d]) / (2 dx_d)` with W_c = velocity_c[f] and W_d the mean of the four d-faces around f; the result has u's
    boundary and face layout. Centred vector `u` with a centred vector `velocity`: `-sum_d velocity_d[i] (U_c[i + e_d] - U_c[i - e_d]) / (2 dx_d)`; the
    result carries the VELOCITY's boundary (advect.py:124). U_c is component c padded with its own extrapolation. A batch of 1 on either side is shared.
    Differentiable w.r.t. u and the velocity. """
    from . import _capi
    from .field import _cell_grid, _centered_rule, require_plain, same_grid
    require_plain(u, 'advect.differential'); require_plain(velocity, 'advect.differential (velocity)')
    if order != 2:
        raise NotImplementedError(f"HIP backend: advect.differential implements order=2 only (got order={order}); pass order=2")
    if implicit is not None:
        raise NotImplementedError("HIP backend: advect.differential computes explicit stencils only; pass implicit=None")
    if u.spatial_rank not in (2, 3):
        raise NotImplementedError(f"HIP backend: advect.differential on {u.spatial_rank}-D grids is not implemented (2-D and 3-D only)")
    if u.is_centered and not u.is_vector:
        raise NotImplementedError("HIP backend: advect.differential of a centred SCALAR field is not implemented (the reference iterates `u.vector`); advect "
                                  "scalars with advect.semi_lagrangian / mac_cormack, or pass a vector field")
    if velocity.is_staggered != u.is_staggered or (velocity.is_centered and not velocity.is_vector) or not same_grid(u, velocity):
        raise NotImplementedError("HIP backend: advect.differential needs u and velocity of the same kind (both StaggeredGrid or both centred vector fields) "
                                  "on the same grid; resample one with `@` first")
    assert u.dtype == velocity.dtype, "u and velocity must have the same precision"
    be = velocity.backend
    B = max(u.batch_size, velocity.batch_size)
    assert u.batch_size in (1, B) and velocity.batch_size in (1, B), f"batch sizes {u.batch_size} and {velocity.batch_size} do not match"
    batched = u.batched or velocity.batched
    same = u is velocity
    if u.is_staggered:
        if [tuple(a.shape[1:]) for a in u.values] != [tuple(b.shape[1:]) for b in velocity.values] or \
                resolve(u.boundary, u.dims) != resolve(velocity.boundary, velocity.dims):
            raise NotImplementedError("HIP backend: advect.differential of a StaggeredGrid needs u to share the velocity's boundary conditions; "
                                      "`u.with_boundary(velocity.boundary)` re-stores it")
        grid = velocity.grid_struct(batch=B)
        uv = [t.contiguous() for t in u.values]
        vv = uv if same else [t.contiguous() for t in velocity.values]
        if autodiff.needs_grad(*uv, *vv):
            meta = dict(be=be, grid=grid, rank=u.spatial_rank, same=same)
            args = uv if same else [_expand(t, B) for t in uv] + [_expand(t, B) for t in vv]
            out = list(autodiff.AdvectDifferentialStaggered.apply(meta, *args))
        else:
            out = [be.empty((B,) + tuple(t.shape[1:]), u.dtype) for t in uv]
            be.ctx.advect_differential(grid, _ptrs(uv), u.batch_size, _ptrs(vv), velocity.batch_size, _ptrs(out), be.stream())
        return Field(u.resolution, u.bounds, u.boundary, out, True, be, batched)
    s_codes, s_val = _centered_rule(u, 'advect.differential')
    grid = _cell_grid(u, B)
    src = u.values.contiguous()
    vel = src if same else velocity.values.contiguous()
    if autodiff.needs_grad(src, vel):
        meta = dict(be=be, grid=grid, s_codes=s_codes, s_val=s_val, same=same)
        out = autodiff.AdvectDifferentialCentered.apply(meta, *([src] if same else [_expand(src, B), _expand(vel, B)]))
    else:
        out = be.empty((B,) + tuple(src.shape[1:]), u.dtype)
        be.ctx.advect_differential_centered(grid, src.data_ptr(), u.batch_size, s_codes, s_val, vel.data_ptr(), velocity.batch_size, out.data_ptr(), be.stream())
    return Field(velocity.resolution, velocity.bounds, velocity.boundary, out, False, be, batched, vector=True)


finite_difference = differential


def mac_cormack(field: Field, velocity: Field, dt: float, correction_strength=1.0, integrator: Callable = euler) -> Field:
    """ MacCormack advection (phi/physics/advect.py:182-215): forward + backward semi-Lagrangian lookups estimate the first-order
    error, the corrected value is clamped to the grid values around the backward lookup.

    Args:
        field: `CenteredGrid` or `StaggeredGrid` to be advected
        velocity: `StaggeredGrid` on the same grid
        dt: time increment
        correction_strength: factor on the error estimate (0 = semi-Lagrangian)
        integrator: `euler` (fused kernels), `rk4` or `finite_rk4` (general sampling path; centred fields only)
    """
    return _advect(field, velocity, dt, integrator, float(correction_strength))


def _expand(t: torch.Tensor, B: int) -> torch.Tensor:
    if t.shape[0] == B:
        return t.contiguous()
    assert t.shape[0] == 1
    return t.expand(B, *t.shape[1:]).contiguous()

"""
Explicit and implicit diffusion on the HIP backend (reference: phi/physics/diffuse.py:13-92).
The diffusivity is a number, a per-axis vector (`vec(x=1, y=2)` or a tuple), a centred `Field` (Heat_Flow.ipynb's conductivity) or a
lazy `field * (k_x, k_y)`; the last three run on the flux-form kernels of csrc/diffuse_coef.hpp.
"""
import warnings
from typing import List, Optional, Sequence

import torch

from . import autodiff
from .extrapolation import ConstantExtrapolation, resolve
from .field import Field, _ptrs


def _scalar_walls(f: Field):
    """ (codes, constants) of a centred field's extrapolation for the C ABI (s_bc / s_val) """
    codes, vals = resolve(f.boundary, f.dims)
    val = [[vals[a][s][0] if isinstance(f.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)] for a, d in enumerate(f.dims)]
    return codes, val


def _fold(u: Field, diffusivity, what: str):
    """ a centred vector field (B, C, *res) as the centred scalar field (B * C, *res) -- a free view -- and its diffusivity with a Field of
    batch B expanded to B * C (entry b * C + c diffuses component c of batch entry b) """
    from .field import require_scalar_boundary
    require_scalar_boundary(u.boundary, u.dims, what)
    B, C = u.batch_size, u.spatial_rank
    folded = Field(u.resolution, u.bounds, u.boundary, u.values.reshape(B * C, *u.values.shape[2:]), False, u.backend, True)
    if isinstance(diffusivity, Field) and diffusivity.is_centered and not diffusivity.is_vector and diffusivity.batch_size > 1:
        if diffusivity.batch_size != B:
            raise NotImplementedError(f"{what}: a diffusivity with batch {diffusivity.batch_size} for a field with batch {B}")
        diffusivity = Field(diffusivity.resolution, diffusivity.bounds, diffusivity.boundary, diffusivity.values.repeat_interleave(C, dim=0), False,
                            diffusivity.backend, True, diffusivity.vector_scale)
    return folded, diffusivity


def _unfold(u: Field, result: Field) -> Field:
    out = Field(u.resolution, u.bounds, u.boundary, result.values.reshape(u.values.shape), False, u.backend, u.batched, vector=True)
    out.solve_info = result.solve_info
    return out


def _diffusivity(u: Field, diffusivity, what: str):
    """ -> (None, k) for a number (the constant-coefficient path), else (coefficient Field on u's grid or None, per-axis factors [D]).
    A Field that does not live on u's grid is resampled first (`amount.at(u)`, diffuse.py:55-56), keeping its own extrapolation. """
    from .geom import Vector
    if isinstance(diffusivity, Field):
        if u.is_staggered:
            raise NotImplementedError(f"{what}: a Field diffusivity needs a CenteredGrid: spatially varying diffusion is only defined for "
                                      f"centred grids (phi/physics/diffuse.py:138)")
        if diffusivity.is_staggered:
            raise NotImplementedError(f"{what}: the diffusivity must be a CenteredGrid (a scalar per cell), got a StaggeredGrid")
        if autodiff.needs_grad(diffusivity.values):
            raise NotImplementedError(f"{what}: gradients with respect to the diffusivity are not implemented; detach it (stop_gradient)")
        factors = list(diffusivity.vector_scale) if diffusivity.vector_scale is not None else [1.0] * u.spatial_rank
        coef = Field(diffusivity.resolution, diffusivity.bounds, diffusivity.boundary, diffusivity.values, False, diffusivity.backend, diffusivity.batched)
        if coef.dims != u.dims or coef.resolution != u.resolution or tuple(coef.bounds.lower) != tuple(u.bounds.lower) \
                or tuple(coef.bounds.upper) != tuple(u.bounds.upper):
            from . import sampling
            coef = sampling.resample_general(coef, u)
            coef = Field(coef.resolution, coef.bounds, diffusivity.boundary, coef.values, False, coef.backend, coef.batched)
        if coef.batch_size not in (1, u.batch_size):
            raise NotImplementedError(f"{what}: a diffusivity with batch {coef.batch_size} for a field with batch {u.batch_size} (batch-valued "
                                      f"diffusivities are not implemented)")
        return coef, factors
    if isinstance(diffusivity, Vector):
        missing = [d for d in u.dims if d not in diffusivity]
        if missing:
            raise ValueError(f"{what}: the diffusivity vector {dict(diffusivity)} has no component for {missing}")
        factors = [float(diffusivity[d]) for d in u.dims]
    elif isinstance(diffusivity, (tuple, list)):
        if len(diffusivity) != u.spatial_rank:
            raise ValueError(f"{what}: {len(diffusivity)} diffusivities for a {u.spatial_rank}-D field")
        factors = [float(k) for k in diffusivity]
    else:
        return None, float(diffusivity)
    if all(k == factors[0] for k in factors):
        return None, factors[0]             # an isotropic vector is the number: same kernels, same bits
    if u.is_staggered:
        raise NotImplementedError(f"{what}: a per-axis diffusivity needs a CenteredGrid (the reference's laplace(weights=...) of a staggered "
                                  f"field is not implemented here)")
    return None, factors


def explicit(u: Field, diffusivity, dt: float, substeps: int = 1, order: int = 2) -> Field:
    """ Simulate a finite-time diffusion process of the form dF/dt = α · ΔF with explicit Euler steps (`diffuse.explicit`,
    order 2) on a StaggeredGrid or a CenteredGrid. The field's own extrapolation pads the stencil (tangential wall values of a
    velocity matter). Differentiable w.r.t. u (adjoint stencil kernels). `diffusivity`: a number; for a CenteredGrid also a per-axis
    `vec(...)` / tuple, a centred `Field` (resampled to u's grid if it lives elsewhere) or a lazy `Field * (k_x, k_y)` -- the conservative
    flux form of diffuse.py:129-141. """
    from .field import require_plain
    require_plain(u, 'diffuse.explicit')
    if u.is_vector:         # a centred vector field: every component is a centred scalar grid, diffused on its own
        folded, folded_k = _fold(u, diffusivity, 'diffuse.explicit')
        return _unfold(u, explicit(folded, folded_k, dt, substeps, order))
    if order != 2:
        raise NotImplementedError("HIP backend: diffuse.explicit implements order=2 only")
    coef, k = _diffusivity(u, diffusivity, 'diffuse.explicit')
    if coef is not None or isinstance(k, list):
        return _explicit_coef(u, coef, k if isinstance(k, list) else [k] * u.spatial_rank, dt, substeps)
    diffusivity = k
    amount = diffusivity * dt
    # CFL warning of the reference (diffuse.py:49-54)
    ratio = max(amount / substeps / (h * h) for h in u.dx)
    if ratio > 0.5:
        warnings.warn(f"CFL condition violated in diffuse.explicit: dt*diffusivity/dx^2 = {ratio:.3f} > 0.5, consider more substeps",
                      RuntimeWarning)
    be = u.backend
    kdt = amount / substeps
    if u.is_staggered:
        cur = [t.contiguous() for t in u.values]
        tracked = autodiff.needs_grad(*cur)
        for _ in range(substeps):
            if tracked:
                cur = list(autodiff.DiffuseStaggered.apply(dict(be=be, grid=u.grid_struct(), kdt=kdt, dtype=u.dtype), *cur))
            else:
                out = [torch.empty_like(t) for t in cur]
                be.ctx.diffuse_explicit(u.grid_struct(), _ptrs(cur), _ptrs(out), kdt, be.stream())
                cur = out
        return u.with_values(cur)
    s_codes, s_vals = resolve(u.boundary, u.dims)
    s_val = [[s_vals[a][s][0] if isinstance(u.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)]
             for a, d in enumerate(u.dims)]
    # the grid descriptor only carries the cell grid here; periodicity must match the scalar's
    from . import _capi
    from .field import _torch_dtype_code
    grid = _capi.make_grid(u.spatial_rank, _torch_dtype_code(u.dtype), u.batch_size, list(u.resolution.values()), u.bounds.lower, u.bounds.upper,
                           [[0 if c == 0 else 2 for c in pair] for pair in s_codes])
    cur = u.values.contiguous()
    tracked = autodiff.needs_grad(cur)
    for _ in range(substeps):
        if tracked:
            cur = autodiff.DiffuseCentered.apply(dict(be=be, grid=grid, kdt=kdt, s_codes=s_codes, s_val=s_val), cur)
        else:
            out = torch.empty_like(cur)
            be.ctx.diffuse_explicit_centered(grid, cur.data_ptr(), s_codes, s_val, out.data_ptr(), kdt, False, be.stream())
            cur = out
    return u.with_values(cur)


def _explicit_coef(u: Field, coef: Optional[Field], factors: List[float], dt: float, substeps: int) -> Field:
    """ diffuse.explicit with a coefficient field and / or per-axis factors: `substeps` launches of the flux-form stencil (diffuse_coef.hpp) """
    from . import _capi
    from .field import _torch_dtype_code
    from .jit import is_tracing
    kdt = [k * dt / substeps for k in factors]
    # CFL warning of the reference (diffuse.py:48-54): the maximum of the amount over space (a host read: skipped inside a jit_compile trace)
    if not is_tracing():
        amax = float(coef.values.max()) if coef is not None else 1.0
        ratio = max(amax * k / (h * h) for k, h in zip(kdt, u.dx))
        if ratio > 0.5:
            warnings.warn(f"CFL condition violated in diffuse.explicit: max(diffusivity)*dt/dx^2 = {ratio:.3f} > 0.5, consider more substeps",
                          RuntimeWarning)
    be = u.backend
    s_codes, s_val = _scalar_walls(u)
    grid = _capi.make_grid(u.spatial_rank, _torch_dtype_code(u.dtype), u.batch_size, list(u.resolution.values()), u.bounds.lower, u.bounds.upper,
                           [[0 if c == 0 else 2 for c in pair] for pair in s_codes])
    c = coef.values.to(u.dtype).contiguous() if coef is not None else None
    c_codes, c_val = _scalar_walls(coef) if coef is not None else (s_codes, s_val)
    meta = dict(be=be, grid=grid, kdt=kdt, s_codes=s_codes, s_val=s_val, coef=c, c_batch=c.shape[0] if c is not None else 1, c_codes=c_codes, c_val=c_val)
    cur = u.values.contiguous()
    tracked = autodiff.needs_grad(cur)
    for _ in range(substeps):
        if tracked:
            cur = autodiff.DiffuseCoefCentered.apply(meta, cur)
        else:
            out = torch.empty_like(cur)
            be.ctx.diffuse_explicit_centered_coef(grid, cur.data_ptr(), s_codes, s_val, c.data_ptr() if c is not None else 0, meta['c_batch'], c_codes,
                                                  c_val, kdt, out.data_ptr(), False, be.stream())
            cur = out
    return u.with_values(cur)


def differential(u: Field, diffusivity, gradient=None, order: int = 2, implicit=None, upwind=None, correct_skew=True) -> Field:
    """ The differential diffusion term d * laplace(u) as it stands on the right-hand side of a PDE (`diffuse.differential`,
    phi/physics/diffuse.py:98-144), order 2. A number -- and for centred fields a per-axis `vec(...)` / tuple -- gives `laplace(u, weights=diffusivity)`
    (the same kernels, the same bits); a centred `Field` diffusivity on a centred `u` the conservative flux form of :129-136, through the operator
    I + L of `diffuse.explicit` with dt = 1 (the term is `explicit(u, d, 1) - u`: one extra rounding of |u + L u| per sample). The result keeps u's
    sample layout and carries `u.boundary - u.boundary` (:141): PERIODIC and ZERO_GRADIENT stay, a constant becomes ZERO. Differentiable w.r.t. u.
    `gradient`, `upwind` and `correct_skew` belong to the reference's mesh branch and are not read. """
    from .field import _difference_extrapolation, _laplace_on_lattice, require_plain
    require_plain(u, 'diffuse.differential')
    if order != 2:
        raise NotImplementedError("HIP backend: diffuse.differential implements order=2 only")
    if implicit is not None:
        raise NotImplementedError("HIP backend: diffuse.differential computes the explicit stencil only; pass implicit=None (diffuse.implicit solves)")
    ext = _difference_extrapolation(u.boundary, u.dims)
    coef, k = _diffusivity(u, diffusivity, 'diffuse.differential')
    if coef is not None:
        with warnings.catch_warnings():         # (dt = 1 is no time step: the CFL warning of diffuse.explicit does not apply to a right-hand side)
            warnings.simplefilter('ignore', RuntimeWarning)
            lap = explicit(u, diffusivity, 1.0) - u
    else:
        lap = _laplace_on_lattice(u, None, tuple(k) if isinstance(k, list) else k, 2)
    return Field(u.resolution, u.bounds, ext, lap.values, u.is_staggered, u.backend, lap.batched, vector=u.is_vector)


finite_difference = differential


def implicit(field: Field, diffusivity, dt: float, solve=None, order: int = 2) -> Field:
    """ Implicit Euler diffusion (`diffuse.implicit`, phi/physics/diffuse.py:63-92; Heat_Flow.ipynb, Burgers.ipynb): solves
    `(1 - diffusivity * dt * laplace) u = field` with CG from `x0 = field` -- `solve_linear(sharpen, y=field, solve)` with
    `sharpen(x) = explicit(x, diffusivity, -dt)`. The solver is the matrix-free CG of the pressure path (same kernels, operator
    I - k dt L) on the field's own lattice and extrapolation; every component of a StaggeredGrid is solved separately (the
    operator does not couple them). `solve`: `Solve('CG' | 'CG-adaptive', rel_tol, abs_tol, max_iterations)`; raises
    `NotConverged` / `Diverged` like `solve_linear` unless suppressed. Differentiable w.r.t. the field: the operator is symmetric, the
    backward pass is one more solve (with `solve.gradient_solve` if given) of the same system with homogeneous boundary constants.
    A centred VECTOR field is solved as one CG per (batch entry, component) on the (B * C, *res) view; its SolveInfo lists them batch-major.
    PhiML solves the stacked vector as one system: per-component convergence (|r_c| <= rel |y_c| for every c) implies the joint criterion,
    so a converged result passes the reference's stopping test, but the iterates (and the iteration counts) differ.
    `diffusivity` takes the forms of `explicit`; a Field or per-axis one runs the CG of csrc/diffuse_coef.hpp on sharpen = I + L_{-dt a}. """
    from .field import require_plain, _torch_dtype_code
    from .solve import Solve, SolveInfo
    from .jit import is_tracing
    traced = is_tracing()       # inside a jit_compile'd function: info = NULL, no host read-back, nothing raised (jit.py)
    from .fluid import _raise_if_failed
    from . import _capi
    require_plain(field, 'diffuse.implicit')
    if field.is_vector:     # one CG per (batch entry, component); SolveInfo lists them batch-major (entry b * C + c)
        folded, folded_k = _fold(field, diffusivity, 'diffuse.implicit')
        return _unfold(field, implicit(folded, folded_k, dt, solve, order))
    if order != 2:
        raise NotImplementedError("HIP backend: diffuse.implicit implements order=2 only")
    solve = Solve('CG') if solve is None else solve
    if solve.preconditioner is not None or (solve.gradient_solve is not None and solve.gradient_solve.preconditioner is not None):
        raise NotImplementedError("HIP backend: diffuse.implicit takes no preconditioner (Solve(preconditioner='multigrid') covers the pressure solve only)")
    if solve.x0 is not None:
        raise NotImplementedError("HIP backend: diffuse.implicit starts from x0 = field (the reference's default); pass solve.x0=None")
    vals = field.values if field.is_staggered else [field.values]
    tracked = autodiff.needs_grad(*vals)
    be = field.backend
    fp64 = field.dtype == torch.float64
    csolve = solve.to_c(fp64)
    if traced:
        csolve.check_every = 0
        if tracked:
            raise NotImplementedError("HIP backend: gradients through a jit_compile'd function are not implemented")
    csolve_bwd = (solve.gradient_solve or solve).to_c(fp64)
    coef, k = _diffusivity(field, diffusivity, 'diffuse.implicit')
    if coef is not None or isinstance(k, list):
        factors = k if isinstance(k, list) else [k] * field.spatial_rank
        kdt = [f * float(dt) for f in factors]
        s_codes, s_val = _scalar_walls(field)
        grid = _capi.make_grid(field.spatial_rank, _torch_dtype_code(field.dtype), field.batch_size, list(field.resolution.values()), field.bounds.lower,
                               field.bounds.upper, [[0 if c == 0 else 2 for c in pair] for pair in s_codes])
        c = coef.values.to(field.dtype).contiguous() if coef is not None else None
        c_codes, c_val = _scalar_walls(coef) if coef is not None else (s_codes, s_val)
        meta = dict(be=be, grid=grid, kdt=kdt, s_codes=s_codes, s_val=s_val, coef=c, c_batch=c.shape[0] if c is not None else 1, c_codes=c_codes,
                    c_val=c_val, csolve=csolve, csolve_bwd=csolve_bwd)
        cur = field.values.contiguous()
        if tracked:
            out = autodiff.DiffuseImplicitCoefCentered.apply(meta, cur)
            infos = meta['infos']
        else:
            out = torch.empty_like(cur)
            infos = be.ctx.diffuse_implicit_centered_coef(grid, cur.data_ptr(), s_codes, s_val, c.data_ptr() if c is not None else 0, meta['c_batch'],
                                                          c_codes, c_val, kdt, out.data_ptr(), csolve, be.stream(), want_info=not traced)
        result = field.with_values(out)
        return _finish_implicit(result, infos, solve)
    kdt = float(k) * float(dt)
    if field.is_staggered:
        cur = [t.contiguous() for t in field.values]
        if tracked:
            meta = dict(be=be, grid=field.grid_struct(), kdt=kdt, dtype=field.dtype, csolve=csolve, csolve_bwd=csolve_bwd)
            out = list(autodiff.DiffuseImplicitStaggered.apply(meta, *cur))
            infos = meta['infos']
        else:
            out = [torch.empty_like(t) for t in cur]
            infos = be.ctx.diffuse_implicit(field.grid_struct(), _ptrs(cur), _ptrs(out), kdt, csolve, be.stream(), want_info=not traced)
        result = field.with_values(out)
    else:
        s_codes, s_vals = resolve(field.boundary, field.dims)
        s_val = [[s_vals[a][s][0] if isinstance(field.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)]
                 for a, d in enumerate(field.dims)]
        grid = _capi.make_grid(field.spatial_rank, _torch_dtype_code(field.dtype), field.batch_size, list(field.resolution.values()), field.bounds.lower,
                               field.bounds.upper, [[0 if c == 0 else 2 for c in pair] for pair in s_codes])
        cur = field.values.contiguous()
        if tracked:
            meta = dict(be=be, grid=grid, kdt=kdt, s_codes=s_codes, s_val=s_val, csolve=csolve, csolve_bwd=csolve_bwd)
            out = autodiff.DiffuseImplicitCentered.apply(meta, cur)
            infos = meta['infos']
        else:
            out = torch.empty_like(cur)
            infos = be.ctx.diffuse_implicit_centered(grid, cur.data_ptr(), s_codes, s_val, out.data_ptr(), kdt, csolve, be.stream(), want_info=not traced)
        result = field.with_values(out)
    return _finish_implicit(result, infos, solve)


def _finish_implicit(result: Field, infos, solve) -> Field:
    """ solve_linear semantics: NotConverged / Diverged unless suppressed; the SolveInfo rides on the result (no infos: traced, nothing read back) """
    from .solve import SolveInfo
    from .fluid import _raise_if_failed
    if infos is not None:
        info = SolveInfo(solve, [i.iterations for i in infos], [i.residual_sq for i in infos], [i.rhs_sq for i in infos],
                         [bool(i.converged) for i in infos], [bool(i.diverged) for i in infos])
        _raise_if_failed(info)
        result.solve_info = info
    return result

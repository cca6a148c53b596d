"""
`Field` / `CenteredGrid` / `StaggeredGrid`: the host-side mirror of PhiFlow's grid fields
(reference: phi/field/_field.py:51-211, phi/field/_grid.py:21-176, phi/geom/_grid.py:41-122,204-209).

Only uniform grids are supported. A field owns device tensors (torch, ROCm) laid out exactly as the C ABI wants them:
  * CenteredGrid  -> one tensor (batch, x, y[, z]); a centred VECTOR field (`is_vector`) -> one tensor (batch, D, x, y[, z]), component-major:
    component c of batch entry b is a contiguous centred scalar grid, so (batch * D, *res) is a free view for the scalar kernels
  * StaggeredGrid -> one tensor per component d with shape (batch, *res + (lo+up-1) e_d)   (faces stored iff
    `boundary.valid_outer_faces(d)`, tests/commit/field/test__grid.py:25-36)
Fields are immutable from the user's point of view: every operator returns new fields (phi/field/_field.py:49-51).
PhiML's named batch dims are reduced to ONE leading batch dimension (size 1 when the field is not batched).
"""
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from .backend import HipBackend, default_backend, float_dtype
from .extrapolation import BOUNDARY, PERIODIC, ZERO, ConstantExtrapolation, Extrapolation, as_extrapolation, resolve
from .geom import Box, Geometry, Vector
from .noise import Noise


def _torch_dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return _capi.PHIHIP_F32
    if dtype == torch.float64:
        return _capi.PHIHIP_F64
    raise TypeError(f"unsupported dtype {dtype}; the HIP backend computes in float32 or float64")


_GRID_CACHE = {}      # (id of the resolved boundary codes, dtype, batch, resolution, lower, upper) -> (phihip_grid, codes): Field.grid_struct


class Field:
    """ A sampled grid field with boundary conditions: a centred scalar, a centred vector (`is_vector`) or a staggered vector. """
    __array_ufunc__ = None     # `numpy_array * field` defers to Field.__rmul__ (a batch vector, one number per batch entry)
    solve_info = None          # set on the pressure that a solve returns (solve.SolveInfo); None on every other field and on results of a captured function (jit.py)

    def __init__(self, resolution: Dict[str, int], bounds: Box, boundary: Extrapolation, values, staggered: bool,
                 backend: HipBackend, batched: bool, vector_scale: Optional[Sequence[float]] = None, vector: bool = False):
        # vector_scale: `scalar * (0, 0.1)` -- a centred scalar times a constant vector, kept lazily (values stay the scalar's) until
        # it is resampled to a staggered grid with `@` / `resample`. Arithmetic and resample carry it along; every other consumer of
        # `values` (mean, gradients, divergence, advection, diffusion, losses, file output) calls `require_plain` and refuses
        assert vector_scale is None or (not staggered and not vector and len(vector_scale) == len(resolution))
        assert not (vector and staggered)
        self.is_vector = bool(vector)      # centred vector field: values (batch, D, *res)
        self.vector_scale = [float(c) for c in vector_scale] if vector_scale is not None else None
        self.resolution = dict(resolution)
        self._dims = tuple(self.resolution)
        self.bounds = bounds
        self.boundary = boundary
        self.values = values           # Tensor (centred) or List[Tensor] (staggered)
        self.is_staggered = staggered
        self.backend = backend
        self.batched = batched
        self._codes, self._bc_val = resolve(boundary, self.dims)

    # --- geometry -------------------------------------------------------------------------------------------------
    @property
    def dims(self) -> Tuple[str, ...]:
        return self._dims

    @property
    def spatial_rank(self) -> int:
        return len(self.resolution)

    @property
    def extrapolation(self) -> Extrapolation:
        return self.boundary

    @property
    def is_centered(self) -> bool:
        return not self.is_staggered

    @property
    def is_grid(self) -> bool:
        return True

    @property
    def dx(self) -> Tuple[float, ...]:
        return tuple(s / r for s, r in zip(self.bounds.size, self.resolution.values()))

    @property
    def dtype(self) -> torch.dtype:
        return (self.values[0] if self.is_staggered else self.values).dtype

    @property
    def batch_size(self) -> int:
        return int((self.values[0] if self.is_staggered else self.values).shape[0])

    @property
    def shape(self):
        """ (batch, *resolution) -- for staggered fields the per-component shapes are in `component_shapes` """
        return (self.batch_size,) + tuple(self.resolution.values())

    @property
    def component_shapes(self) -> List[Tuple[int, ...]]:
        return [component_shape(self.resolution, self.boundary, d) for d in range(self.spatial_rank)]

    def grid_struct(self, batch: Optional[int] = None, dtype: Optional[torch.dtype] = None) -> _capi.Grid:
        """ the `phihip_grid` descriptor of this field's grid + boundary """
        # r6: the descriptor is built once per (grid, boundary, dtype, batch) and reused by every Field on it (an eager 128^2 plume step built four per step,
        # 13 us each, out of ~0.2 ms of host work; nothing mutates a Grid after make_grid). `_codes` is the list cached on the extrapolation object (resolve).
        key = (id(self._codes), _torch_dtype_code(dtype or self.dtype), batch or self.batch_size, tuple(self.resolution.values()),
               tuple(self.bounds.lower), tuple(self.bounds.upper))
        hit = _GRID_CACHE.get(key)
        if hit is not None and hit[1] is self._codes:
            return hit[0]
        g = _capi.make_grid(self.spatial_rank, key[1], key[2], key[3], key[4], key[5], self._codes, self._bc_val)
        if len(_GRID_CACHE) >= 512:
            _GRID_CACHE.clear()
        _GRID_CACHE[key] = (g, self._codes)
        return g

    # --- access ---------------------------------------------------------------------------------------------------
    def numpy(self):
        """ host copy; batch dim squeezed when the field is not batched. Staggered: list of component arrays. Centred vector: channel-last
        (*res, D) like the constructor takes it (PhiML's order: spatial, then vector). """
        def conv(t):
            a = t.detach().cpu().numpy()
            return a if self.batched else a[0]
        if self.is_vector:
            return conv(torch.movedim(self.values, 1, -1))
        return [conv(t) for t in self.values] if self.is_staggered else conv(self.values)

    def __getitem__(self, item) -> 'Field':
        """ `v['x']`: component as a centred field on its staggered sub-grid (phi/field/_field.py:657-689); of a centred vector field the
        component as a centred scalar field on the same grid """
        if self.is_vector and item in self.dims:
            return Field(self.resolution, self.bounds, self.boundary, self.values[:, self.dims.index(item)], False, self.backend, self.batched)
        assert self.is_staggered and item in self.dims, f"can only select a vector component of a staggered field, got {item!r}"
        d = self.dims.index(item)
        lo, up = self.boundary.valid_outer_faces(item)
        dx = self.dx[d]
        kw = {dim: (l, u) for dim, l, u in zip(self.dims, self.bounds.lower, self.bounds.upper)}
        kw[item] = (self.bounds.lower[d] + (-0.5 if lo else 0.5) * dx, self.bounds.upper[d] + (0.5 if up else -0.5) * dx)
        res = dict(self.resolution)
        res[item] = self.values[d].shape[1 + d]
        comp_boundary = self.boundary
        return Field(res, Box(**kw), comp_boundary, self.values[d], False, self.backend, self.batched)

    def with_values(self, values) -> 'Field':
        return Field(self.resolution, self.bounds, self.boundary, values, self.is_staggered, self.backend, self.batched, self.vector_scale, self.is_vector)

    def with_boundary(self, boundary) -> 'Field':
        """ change the extrapolation; staggered fields re-store their boundary faces accordingly: faces that become
        stored take the OLD boundary value (0 on walls), faces determined by the new boundary are dropped
        (phi/field/_field.py:451-472; tests/commit/field/test__grid.py:85-94). """
        boundary = as_extrapolation(boundary)
        if not self.is_staggered:
            return Field(self.resolution, self.bounds, boundary, self.values, False, self.backend, self.batched, self.vector_scale, self.is_vector)
        new_vals = []
        for d, dim in enumerate(self.dims):
            t = self.values[d]
            lo_old, up_old = self.boundary.valid_outer_faces(dim)
            lo_new, up_new = boundary.valid_outer_faces(dim)
            ax = 1 + d
            n = self.resolution[dim]
            # bake to all n+1 faces first
            parts = []
            if not lo_old:
                parts.append(_boundary_slab(t, ax, self._codes[d][0], self._bc_val[d][0][d], lower=True, periodic_src=None))
            parts.append(t)
            if not up_old:
                parts.append(_boundary_slab(t, ax, self._codes[d][1], self._bc_val[d][1][d], lower=False,
                                            periodic_src=parts[0] if lo_old is False else t))
            full = torch.cat(parts, dim=ax) if len(parts) > 1 else t
            assert full.shape[ax] == n + 1
            start = 0 if lo_new else 1
            stop = n + 1 if up_new else n
            new_vals.append(full.narrow(ax, start, stop - start).contiguous())
        return Field(self.resolution, self.bounds, boundary, new_vals, True, self.backend, self.batched)

    with_extrapolation = with_boundary

    # --- arithmetic (elementwise glue on device tensors; not part of the kernel hot path) --------------------------
    def _op(self, other, fn, additive: bool = False) -> 'Field':
        """ elementwise `fn(self, other)`. additive: + / - (a lazy `scalar * vector` field only combines with one of the same vector) """
        scale = self.vector_scale
        vector = self.is_vector
        if isinstance(other, Field) and (self.is_vector or other.is_vector):
            # centred vector with a centred vector, or with a centred scalar (broadcast over the components)
            assert self.is_centered and other.is_centered and same_grid(self, other), \
                f"incompatible fields (sample points differ): {self!r} vs {other!r}; resample one with `@` first"
            if self.vector_scale is not None or other.vector_scale is not None:
                raise NotImplementedError("combining a centred vector field with a lazy `scalar * vector` field; resample it with "
                                          "`field @ vector_field` first")
            a = self.values if self.is_vector else self.values.unsqueeze(1)
            b = other.values if other.is_vector else other.values.unsqueeze(1)
            return Field(self.resolution, self.bounds, self.boundary, fn(a, b), False, self.backend, self.batched or other.batched, None, True)
        if isinstance(other, Field):
            assert other.is_staggered == self.is_staggered and same_grid(self, other), \
                f"incompatible fields (sample points differ): {self!r} vs {other!r}; resample one with `@` first"
            if additive and scale != other.vector_scale:
                raise NotImplementedError("adding a lazy `scalar * vector` field to a field with a different (or no) vector factor; "
                                          "resample it to the staggered grid first (`field @ velocity`)")
            if not additive and other.vector_scale is not None:
                scale = other.vector_scale if scale is None else [a * b for a, b in zip(scale, other.vector_scale)]
            if self.is_staggered:
                assert [tuple(a.shape[1:]) for a in self.values] == [tuple(b.shape[1:]) for b in other.values], \
                    "staggered fields with different face layouts (boundaries) cannot be combined"
                vals = [fn(a, b) for a, b in zip(self.values, other.values)]
            else:
                vals = fn(self.values, other.values)
            batched = self.batched or other.batched
        elif isinstance(other, (tuple, list)) and self.is_vector:
            assert len(other) == self.spatial_rank, f"vector operand of length {len(other)} for a {self.spatial_rank}-D vector field"
            w = torch.as_tensor([float(c) for c in other], dtype=self.dtype, device=self.backend.device).reshape(1, -1, *([1] * self.spatial_rank))
            vals = fn(self.values, w)
            batched = self.batched
        elif isinstance(other, (tuple, list)):
            assert self.is_staggered and len(other) == self.spatial_rank, "vector operand requires a staggered field"
            vals = [fn(a, float(c)) for a, c in zip(self.values, other)]
            batched = self.batched
        elif additive and scale is not None:
            raise NotImplementedError("adding a number to a lazy `scalar * vector` field; resample it to the staggered grid first")
        elif isinstance(other, (np.ndarray, torch.Tensor)) and other.ndim == 1:
            # one number per batch entry, e.g. `inflow_rate * resample(inflow, to=s, soft=True)` (Batched_Smoke.ipynb)
            assert self.batch_size in (1, len(other)), f"batch vector of length {len(other)} does not match batch size {self.batch_size}"
            w = torch.as_tensor(np.asarray(other) if isinstance(other, np.ndarray) else other, dtype=self.dtype, device=self.backend.device)
            w = w.reshape(-1, *([1] * (self.spatial_rank + int(self.is_vector))))
            vals = [fn(a, w) for a in self.values] if self.is_staggered else fn(self.values, w)
            batched = True
        else:
            vals = [fn(a, other) for a in self.values] if self.is_staggered else fn(self.values, other)
            batched = self.batched
        return Field(self.resolution, self.bounds, self.boundary, vals, self.is_staggered, self.backend, batched, scale, vector)

    def __add__(self, other): return self._op(other, lambda a, b: a + b, additive=True)
    def __radd__(self, other): return self._op(other, lambda a, b: b + a, additive=True)
    def __sub__(self, other): return self._op(other, lambda a, b: a - b, additive=True)
    def __rsub__(self, other): return self._op(other, lambda a, b: b - a, additive=True)
    def __mul__(self, other):
        if isinstance(other, (tuple, list)) and self.is_centered and not self.is_vector:
            return vector_scaled(self, other)   # `smoke * (0, 0.1)`; becomes a vector field when resampled with `@`
        return self._op(other, lambda a, b: a * b)

    def __rmul__(self, other): return self.__mul__(other)
    def __truediv__(self, other):
        if isinstance(other, Field) and other.vector_scale is not None:
            raise NotImplementedError("division by a lazy `scalar * vector` field")
        return self._op(other, lambda a, b: a / b)
    def __neg__(self): return self._op(-1.0, lambda a, b: a * b)

    def __pow__(self, exponent):
        """ `u ** 2` (a number exponent, elementwise; Reaction_Diffusion.ipynb's `u * v ** 2`) """
        if not isinstance(exponent, (int, float)):
            raise NotImplementedError(f"Field ** {type(exponent).__name__}: only number exponents are implemented")
        require_plain(self, '**')
        return self._op(exponent, lambda a, b: a ** b)

    def laplace(self, axes=None, weights=None, order: int = 2) -> 'Field':
        return laplace(self, axes, weights, order)

    def divergence(self, order: int = 2) -> 'Field':
        return divergence(self, order)

    def gradient(self, boundary=None, at: str = 'center', order: int = 2) -> 'Field':
        """ `field.gradient(boundary, at, order)` (phi/field/_field.py `Field.gradient`): `spatial_gradient` as a method, with the reference's default location
        'center' (the function's default here stays 'face') """
        return spatial_gradient(self, boundary, at=at, order=order)

    @property
    def sampled_at(self) -> str:
        """ 'face' for a StaggeredGrid, 'center' for a CenteredGrid (phi/field/_field.py `Field.sampled_at`) """
        return 'face' if self.is_staggered else 'center'

    def curl(self, at: str = 'corner') -> 'Field':
        return curl(self, at)

    def at_centers(self) -> 'Field':
        """ `field.at_centers()`: the field sampled at the cell centres of its grid -- a centred vector field for a staggered one
        (phi/field/_field.py, _resample.py:241-259), the field itself when it is centred """
        if self.is_centered:
            return self
        target = torch.zeros((1,) + tuple(self.resolution.values()), dtype=self.dtype, device=self.backend.device)
        return resample(self, to=Field(self.resolution, self.bounds, self.boundary, target, False, self.backend, False))

    def __matmul__(self, other: 'Field') -> 'Field':
        """ `value @ target`: resample to the sample points of `target`, keeping `target`'s boundary
        (phi/field/_field.py `__matmul__` -> resample). """
        return resample(self, to=other)

    def __repr__(self):
        kind = "StaggeredGrid" if self.is_staggered else ("CenteredGrid(vector)" if self.is_vector else "CenteredGrid")
        return f"{kind}[{self.resolution}, batch={self.batch_size if self.batched else None}, {self.boundary}, {self.dtype}, {self.backend}]"


def require_plain(field, what: str):
    """ refuse a lazily vector-scaled scalar (`smoke * (0, 0.1)`) where its `values` would be taken for the field itself: the result would
    silently be that of the plain scalar. Resample it to a staggered grid first (`field @ velocity`). """
    if isinstance(field, Field) and field.vector_scale is not None:
        raise NotImplementedError(f"{what}: the field is a scalar times the constant vector {tuple(field.vector_scale)} (a centred VECTOR field, not "
                                  f"stored as such); resample it to a StaggeredGrid with `field @ velocity` / `resample(field, to=velocity)` first")


def require_scalar_boundary(boundary: Extrapolation, dims, what: str):
    """ a centred vector field shares ONE extrapolation among its components: vector-valued constants (`vec(x=1, y=0)`) are not implemented """
    for d in dims:
        for upper in (False, True):
            side = boundary.side(d, upper)
            if isinstance(side, ConstantExtrapolation) and isinstance(side.value, (dict, tuple, list)):
                raise NotImplementedError(f"{what}: a vector-valued constant extrapolation ({side}) of a centred vector field is not implemented; "
                                          f"use a number, ZERO_GRADIENT or PERIODIC")


def require_centered_scalar(field, what: str):
    """ refuse a centred vector field where only scalars (or staggered vectors) are implemented """
    if isinstance(field, Field) and field.is_vector:
        raise NotImplementedError(f"{what} of a centred vector field (CenteredGrid with a vector axis) is not implemented")


def same_grid(a: 'Field', b: 'Field') -> bool:
    """ same sample points up to staggering: resolution, bounds and dims (the reference short-circuits `resample` only when
    `value.geometry == to.geometry`, phi/field/_resample.py:42-48) """
    return a.resolution == b.resolution and a.dims == b.dims and tuple(a.bounds.lower) == tuple(b.bounds.lower) \
        and tuple(a.bounds.upper) == tuple(b.bounds.upper)


def _boundary_slab(t: torch.Tensor, ax: int, code: int, const: float, lower: bool, periodic_src) -> torch.Tensor:
    """ one layer of boundary faces along tensor axis `ax` for a normal velocity component """
    if code == _capi.BC_CLOSED:
        shp = list(t.shape)
        shp[ax] = 1
        return torch.full(shp, const, dtype=t.dtype, device=t.device)
    if code == _capi.BC_PERIODIC:
        return t.narrow(ax, 0, 1) if not lower else t.narrow(ax, t.shape[ax] - 1, 1)
    return t.narrow(ax, 0 if lower else t.shape[ax] - 1, 1)


def component_shape(resolution: Dict[str, int], boundary: Extrapolation, d: int) -> Tuple[int, ...]:
    dims = list(resolution.keys())
    lo, up = boundary.valid_outer_faces(dims[d])
    shape = list(resolution.values())
    shape[d] += int(lo) + int(up) - 1
    return tuple(shape)


def _resolve_grid_args(bounds, resolution, resolution_):
    res = dict(resolution or {}, **resolution_)
    assert res, "resolution must be given, e.g. x=64, y=64"
    res = {d: int(r) for d, r in res.items()}
    if bounds is None:
        bounds = Box(**{d: float(r) for d, r in res.items()})   # default: dx = 1 (phi/field/_grid.py:55-60)
    else:
        assert set(bounds.dims) == set(res.keys()), f"bounds {bounds} do not match resolution {res}"
        bounds = Box(**{d: (bounds.lower[bounds.dims.index(d)], bounds.upper[bounds.dims.index(d)]) for d in res})
    return res, bounds


def _sample_points(res: Dict[str, int], bounds: Box, comp: Optional[int], boundary: Extrapolation):
    """ numpy float64 coordinate arrays of cell centres (comp None) or of the stored faces of component `comp` """
    axes = []
    dims = list(res.keys())
    for a, dim in enumerate(dims):
        n = res[dim]
        dx = (bounds.upper[a] - bounds.lower[a]) / n
        if comp is not None and a == comp:
            lo, up = boundary.valid_outer_faces(dim)
            cnt = n + int(lo) + int(up) - 1
            first = 0 if lo else 1
            axes.append(bounds.lower[a] + (first + np.arange(cnt)) * dx)
        else:
            axes.append(bounds.lower[a] + (np.arange(n) + 0.5) * dx)
    return np.meshgrid(*axes, indexing='ij')


def _to_batched(array: np.ndarray, spatial_shape: Tuple[int, ...]) -> Tuple[np.ndarray, bool]:
    array = np.asarray(array)
    if array.shape == tuple(spatial_shape):
        return array[None], False
    if array.ndim == len(spatial_shape) + 1 and array.shape[1:] == tuple(spatial_shape):
        return array, True
    if array.ndim == 0:
        return np.broadcast_to(array, (1,) + tuple(spatial_shape)), False
    raise ValueError(f"values of shape {array.shape} do not match the expected sample shape {spatial_shape} (optionally with a leading batch dim)")


def _tensor_from(value, spatial_shape, backend: HipBackend, dtype) -> Tuple[torch.Tensor, bool]:
    if isinstance(value, torch.Tensor):
        t = value.to(device=backend.device, dtype=dtype)
        if tuple(t.shape) == tuple(spatial_shape):
            return t.unsqueeze(0).contiguous(), False
        assert t.dim() == len(spatial_shape) + 1 and tuple(t.shape[1:]) == tuple(spatial_shape), \
            f"tensor of shape {tuple(t.shape)} does not match sample shape {spatial_shape}"
        return t.contiguous(), True
    arr, batched = _to_batched(value, spatial_shape)
    return backend.as_tensor(np.ascontiguousarray(arr), dtype), batched


def _is_number_vector(values, D: int) -> bool:
    return isinstance(values, (tuple, list)) and len(values) == D and all(isinstance(v, (int, float)) for v in values)


def _vector_tensor_from(value, spatial_shape, backend: HipBackend, dtype) -> Tuple[torch.Tensor, bool]:
    """ an array / tensor with a trailing vector axis, (*res, D) or (batch, *res, D) -> (batch, D, *res), batched """
    D = len(spatial_shape)
    t = value.to(device=backend.device, dtype=dtype) if isinstance(value, torch.Tensor) else backend.as_tensor(np.ascontiguousarray(value, dtype=np.float64), dtype)
    if tuple(t.shape) == tuple(spatial_shape) + (D,):
        return torch.movedim(t, -1, 0).unsqueeze(0).contiguous(), False
    assert t.dim() == D + 2 and tuple(t.shape[1:]) == tuple(spatial_shape) + (D,), \
        f"values of shape {tuple(t.shape)} match neither (batch?, *{spatial_shape}) nor (batch?, *{spatial_shape}, {D})"
    return torch.movedim(t, -1, 1).contiguous(), True


def _fits_scalar(value, spatial_shape) -> bool:
    shp = tuple(np.shape(value)) if not isinstance(value, torch.Tensor) else tuple(value.shape)
    return shp == tuple(spatial_shape) or (len(shp) == len(spatial_shape) + 1 and shp[1:] == tuple(spatial_shape)) or len(shp) == 0


def CenteredGrid(values=0., boundary=0., bounds: Optional[Box] = None, resolution: Optional[Dict[str, int]] = None,
                 batch: Optional[int] = None, backend: Optional[HipBackend] = None, **resolution_) -> Field:
    """ `CenteredGrid(values, boundary, bounds, x=.., y=..)` (phi/field/_grid.py:21-86).
    values: number | array/tensor (optionally with leading batch dim) | callable(*coords) | Geometry (hard mask) | Field | Noise.
    Centred VECTOR fields from: a tuple / list of D numbers or `vec(x=.., y=..)` | a callable returning `vec(x=array, y=array)` | an
    array / tensor with a trailing vector axis (*res, D) or (batch, *res, D) (an array that also fits (batch, *res) keeps that meaning) |
    `Noise(vector='x,y')` | a StaggeredGrid on the same grid (`at_centers`). """
    backend = backend or default_backend()
    boundary = as_extrapolation(boundary)
    res, bounds = _resolve_grid_args(bounds, resolution, resolution_)
    shape = tuple(res.values())
    D = len(shape)
    dtype = float_dtype()
    vector = False
    if isinstance(values, Field) and values.is_staggered:
        assert values.resolution == res
        target = Field(res, bounds, boundary, torch.zeros((1,) + shape, dtype=values.dtype, device=backend.device), False, backend, False)
        t = resample(values, to=target)
        t, batched, vector = t.values.to(dtype), t.batched, True
    elif isinstance(values, Field):
        assert values.is_centered and values.resolution == res
        t, batched, vector = values.values.to(dtype), values.batched, values.is_vector
    elif isinstance(values, Noise):
        vector = values.vector is not None
        if vector:
            assert len(values.vector) == D, f"Noise(vector={values.vector}) on a {D}-D grid"
        t = values.grid_sample(shape, bounds.size, D if vector else 1, backend.device, dtype, values.batch or 1)
        t, batched = (t if vector else t[:, 0]), values.batch is not None
    elif isinstance(values, Geometry):
        pts = _sample_points(res, bounds, None, boundary)
        t, batched = _tensor_from(values.lies_inside(pts).astype(np.float64), shape, backend, dtype)
    elif isinstance(values, Vector) or _is_number_vector(values, D):
        comps = [values[d] for d in res] if isinstance(values, Vector) else list(values)
        arrs = [np.broadcast_to(np.asarray(c, dtype=np.float64), shape) for c in comps]
        t, batched, vector = backend.as_tensor(np.ascontiguousarray(np.stack(arrs)[None]), dtype), False, True
    elif callable(values):
        pts = _sample_points(res, bounds, None, boundary)
        out = values(*pts)
        if isinstance(out, Vector):         # `lambda x, y: vec(x=.., y=..)` (Variable_Boundaries.ipynb)
            arrs = [np.asarray(out[d], dtype=np.float64) for d in res]
            B = max([a.shape[0] for a in arrs if a.shape != shape and a.ndim == D + 1] + [1])
            arrs = [np.broadcast_to(a if a.ndim == D + 1 else a[None], (B,) + shape) for a in arrs]
            t, batched, vector = backend.as_tensor(np.ascontiguousarray(np.stack(arrs, axis=1)), dtype), B > 1, True
        else:
            t, batched = _tensor_from(np.asarray(out, dtype=np.float64), shape, backend, dtype)
    elif isinstance(values, (int, float)):
        t, batched = torch.full((1,) + shape, float(values), dtype=dtype, device=backend.device), False
    elif not _fits_scalar(values, shape) and tuple(np.shape(values) if not isinstance(values, torch.Tensor) else values.shape)[-1:] == (D,):
        t, batched = _vector_tensor_from(values, shape, backend, dtype)
        vector = True
    else:
        t, batched = _tensor_from(values, shape, backend, dtype)
    if vector and D not in (2, 3):
        raise NotImplementedError(f"HIP backend: centred vector fields on {D}-D grids are not implemented (2-D and 3-D only)")
    if batch is not None and t.shape[0] != batch:
        assert t.shape[0] == 1
        t, batched = t.expand(batch, *t.shape[1:]).contiguous(), True
    return Field(res, bounds, boundary, t, False, backend, batched, vector=vector)


def StaggeredGrid(values=0., boundary=0., bounds: Optional[Box] = None, resolution: Optional[Dict[str, int]] = None,
                  batch: Optional[int] = None, backend: Optional[HipBackend] = None, **resolution_) -> Field:
    """ `StaggeredGrid(values, boundary, bounds, x=.., y=..)` (phi/field/_grid.py:89-176).
    values: number | per-component tuple of numbers | list of per-component arrays/tensors | callable(*coords) returning one
    array per component (evaluated at that component's face centres) | Geometry (hard mask at faces) | Field (a centred vector field is
    resampled to the faces) | Noise (every face grid sampled on its own) """
    backend = backend or default_backend()
    boundary = as_extrapolation(boundary)
    res, bounds = _resolve_grid_args(bounds, resolution, resolution_)
    D = len(res)
    dtype = float_dtype()
    shapes = [component_shape(res, boundary, d) for d in range(D)]
    comps, batched = [], False
    if isinstance(values, Field) and values.is_vector:        # centred vector -> faces
        assert values.resolution == res
        target = [torch.zeros((1,) + shp, dtype=values.dtype, device=backend.device) for shp in shapes]   # (lends sample points and dtype)
        return resample(values, to=Field(res, bounds, boundary, target, True, backend, False))
    if isinstance(values, Field):
        assert values.is_staggered and values.resolution == res
        return values.with_boundary(boundary) if values.boundary != boundary else values
    for d in range(D):
        if isinstance(values, Noise):     # every face grid sampled on its own (phi/field/_noise.py:34): cells of size dx, one per stored face
            dx = [(bounds.upper[a] - bounds.lower[a]) / res[k] for a, k in enumerate(res)]
            t = values.grid_sample(shapes[d], [n * h for n, h in zip(shapes[d], dx)], 1, backend.device, dtype, values.batch or 1)[:, 0]
            b = values.batch is not None
        elif isinstance(values, Geometry):
            pts = _sample_points(res, bounds, d, boundary)
            t, b = _tensor_from(values.lies_inside(pts).astype(np.float64), shapes[d], backend, dtype)
        elif callable(values):
            pts = _sample_points(res, bounds, d, boundary)
            out = values(*pts)
            t, b = _tensor_from(np.asarray(out[d], dtype=np.float64), shapes[d], backend, dtype)
        elif isinstance(values, (int, float)):
            t, b = torch.full((1,) + shapes[d], float(values), dtype=dtype, device=backend.device), False
        elif isinstance(values, (tuple, list)) and len(values) == D and all(isinstance(v, (int, float)) for v in values):
            t, b = torch.full((1,) + shapes[d], float(values[d]), dtype=dtype, device=backend.device), False
        elif isinstance(values, (tuple, list)) and len(values) == D:
            t, b = _tensor_from(values[d], shapes[d], backend, dtype)
        else:
            raise ValueError(f"cannot build a StaggeredGrid from {type(values)}")
        comps.append(t)
        batched = batched or b
    B = max(t.shape[0] for t in comps) if batch is None else batch
    if B > 1:
        comps = [t if t.shape[0] == B else t.expand(B, *t.shape[1:]).contiguous() for t in comps]
        batched = True
    return Field(res, bounds, boundary, comps, True, backend, batched)


# ---------------------------------------------------------------------------------------------------------------------
# operators backed by libphihip
# ---------------------------------------------------------------------------------------------------------------------
def _ptrs(tensors: Sequence[torch.Tensor]) -> List[int]:
    return [t.data_ptr() for t in tensors]


def divergence(field: Field, order: int = 2) -> Field:
    """ `field.divergence` of a StaggeredGrid, order 2 (phi/field/_field_math.py:589,617-626) -> CenteredGrid with
    extrapolation `field.extrapolation.spatial_gradient()`; of a centred vector field the central differences of :627-632. """
    require_plain(field, 'divergence')
    if order == 2 and field.is_vector:
        return _divergence_centered(field)
    if order != 2 or not field.is_staggered:
        raise NotImplementedError("the HIP backend implements divergence for a StaggeredGrid or a centred vector field, order=2 only")
    be = field.backend
    vals = [t.contiguous() for t in field.values]
    out = be.empty((field.batch_size,) + tuple(field.resolution.values()), field.dtype)
    be.ctx.divergence(field.grid_struct(), _ptrs(vals), 0, 1, False, out.data_ptr(), be.stream())
    return Field(field.resolution, field.bounds, field.boundary.spatial_gradient(), out, False, be, field.batched)


def spatial_gradient(field: Field, boundary=None, at: str = 'face', order: int = 2) -> Field:
    """ `field.spatial_gradient(p, boundary, at='face')` (phi/field/_field_math.py:148-236): gradient of a centred scalar
    at the faces that a StaggeredGrid with `boundary` stores; `field.boundary` pads p. at='center' (the reference's default; the mirror's stays
    'face'): the central differences of :229-233 as a centred vector field. """
    require_plain(field, 'spatial_gradient')
    require_centered_scalar(field, 'spatial_gradient')
    if at not in ('face', 'center') or order != 2 or field.is_staggered:
        raise NotImplementedError("the HIP backend implements spatial_gradient(at='face' | 'center', order=2) of a scalar CenteredGrid only")
    if at == 'center':
        return _gradient_centered(field, boundary)
    vb = as_extrapolation(boundary if boundary is not None else field.boundary.spatial_gradient())
    be = field.backend
    proto = Field(field.resolution, field.bounds, vb, None, True, be, field.batched)
    grid = _capi.make_grid(field.spatial_rank, _torch_dtype_code(field.dtype), field.batch_size, list(field.resolution.values()),
                           field.bounds.lower, field.bounds.upper, proto._codes, proto._bc_val)
    _check_pressure_padding(field.boundary, vb, field.dims)
    from . import autodiff
    if autodiff.needs_grad(field.values):
        shapes = [(field.batch_size,) + component_shape(field.resolution, vb, d) for d in range(field.spatial_rank)]
        grid_zero = _capi.make_grid(field.spatial_rank, _torch_dtype_code(field.dtype), field.batch_size, list(field.resolution.values()),
                                    field.bounds.lower, field.bounds.upper, proto._codes)
        meta = dict(be=be, grid=grid, grid_zero=grid_zero, shapes=shapes, dtype=field.dtype)
        return Field(field.resolution, field.bounds, vb, list(autodiff.GradientFaces.apply(meta, field.values)), True, be, field.batched)
    comps = [be.zeros((field.batch_size,) + component_shape(field.resolution, vb, d), field.dtype) for d in range(field.spatial_rank)]
    be.ctx.grad_subtract(grid, 0, 1, field.values.contiguous().data_ptr(), _ptrs(comps), be.stream())
    comps = [-c for c in comps]
    return Field(field.resolution, field.bounds, vb, comps, True, be, field.batched)


def _check_pressure_padding(p_ext: Extrapolation, v_ext: Extrapolation, dims):
    from .extrapolation import pressure_extrapolation
    expect = pressure_extrapolation(v_ext, dims)
    for d in dims:
        for upper in (False, True):
            have, want = p_ext.side(d, upper), expect.side(d, upper)
            if type(have) is not type(want) or (isinstance(have, ConstantExtrapolation) and have.component_value(0, d) != 0):
                raise NotImplementedError(f"gradient at faces: scalar extrapolation {have} on side {d}{'+' if upper else '-'} is not the one "
                                          f"the staggered boundary implies ({want}); only the pressure/velocity pairing is implemented")


# ---------------------------------------------------------------------------------------------------------------------
# differential operators at the sample points (csrc/diffops.hpp), order 2
# ---------------------------------------------------------------------------------------------------------------------
def _cell_grid(field: Field, batch: Optional[int] = None) -> _capi.Grid:
    """ descriptor of the cell grid of a centred field: it carries the periodicity only, the field's own rule travels as s_bc / s_val """
    codes = resolve(field.boundary, field.dims)[0]
    return _capi.make_grid(field.spatial_rank, _torch_dtype_code(field.dtype), batch or field.batch_size, list(field.resolution.values()),
                           field.bounds.lower, field.bounds.upper, [[0 if c == 0 else 2 for c in pair] for pair in codes])


def _difference_extrapolation(ext: Extrapolation, dims) -> Extrapolation:
    """ extrapolation of `right - left` of two shifted copies of a field (phi/field/_field.py:791-795): PERIODIC stays, a constant becomes ZERO,
    ZERO_GRADIENT stays (PhiML's rule for the last, recalled: PhiML is not installed) """
    from .extrapolation import _Mixed
    sides = {d: tuple(ZERO if isinstance(ext.side(d, up), ConstantExtrapolation) else ext.side(d, up) for up in (False, True)) for d in dims}
    kinds = {repr(e) for pair in sides.values() for e in pair}
    return next(iter(sides.values()))[0] if len(kinds) == 1 else _Mixed(sides)


def _check_diff_rank(field: Field, what: str):
    if field.spatial_rank not in (2, 3):
        raise NotImplementedError(f"HIP backend: {what} on {field.spatial_rank}-D grids is not implemented (2-D and 3-D only)")


def _laplace_weights(u: Field, axes, weights) -> List[float]:
    """ per-axis factors of the laplace's axis terms: `weights` (None | number | per-axis vec / tuple) on the axes in `axes`, 0 elsewhere """
    if isinstance(weights, Field):
        raise NotImplementedError("laplace: a Field as `weights` is not implemented (a number or a per-axis vec(...) / tuple)")
    if weights is None:
        w = [1.0] * u.spatial_rank
    elif isinstance(weights, Vector):
        missing = [d for d in u.dims if d not in weights]
        if missing:
            raise ValueError(f"laplace: the weights {dict(weights)} have no component for {missing}")
        w = [float(weights[d]) for d in u.dims]
    elif isinstance(weights, (tuple, list)):
        if len(weights) != u.spatial_rank:
            raise ValueError(f"laplace: {len(weights)} weights for a {u.spatial_rank}-D field")
        w = [float(k) for k in weights]
    else:
        w = [float(weights)] * u.spatial_rank
    if axes is None or callable(axes):        # (`spatial`: every axis)
        return w
    names = [a.strip() for a in axes.split(',')] if isinstance(axes, str) else list(axes)
    unknown = [a for a in names if a not in u.dims]
    if unknown:
        raise ValueError(f"laplace: axes {unknown} are not dimensions of {u!r}")
    return [k if d in names else 0.0 for k, d in zip(w, u.dims)]


def laplace(u: Field, axes=None, weights=None, order: int = 2) -> Field:
    """ `field.laplace(u, axes, weights)` (phi/field/_field_math.py:46-145, grid branch :119-145), order 2:
    sum over the axes of w_d (U[i + e_d] + U[i - e_d] - 2 U[i]) / dx_d^2 on every lattice of the field -- a centred scalar, every component of a
    centred vector field, every component of a StaggeredGrid on its own faces with that component's wall constant -- U being the field padded
    with its own extrapolation. Result: the same kind of field with `u.extrapolation.spatial_gradient().spatial_gradient()`.
    Per-axis weights and axis subsets are for centred fields. Differentiable w.r.t. u. """
    out = _laplace_on_lattice(u, axes, weights, order)
    # (a staggered result re-stores its faces: BOUNDARY -> ZERO drops the outer ones, _field_math.py:145)
    return out.with_boundary(u.boundary.spatial_gradient().spatial_gradient())


def _laplace_on_lattice(u: Field, axes, weights, order: int) -> Field:
    """ the values of `laplace` as a field with u's OWN boundary and sample layout (`laplace` and `diffuse.differential` give it their extrapolation) """
    from . import autodiff
    require_plain(u, 'laplace')
    if order != 2:
        raise NotImplementedError("HIP backend: laplace implements order=2 only")
    w = _laplace_weights(u, axes, weights)
    be = u.backend
    if u.is_staggered:
        if any(k != w[0] for k in w):
            raise NotImplementedError("laplace: per-axis weights / an axis subset need a CenteredGrid (as in diffuse)")
        vals = [t.contiguous() for t in u.values]
        if autodiff.needs_grad(*vals):
            out = list(autodiff.LaplaceStaggered.apply(dict(be=be, grid=u.grid_struct(), weight=w[0]), *vals))
        else:
            out = [be.empty(tuple(t.shape), u.dtype) for t in vals]
            be.ctx.field_laplace(u.grid_struct(), _ptrs(vals), _ptrs(out), w[0], False, be.stream())
        return u.with_values(out)
    _check_diff_rank(u, 'laplace')
    if u.is_vector:
        require_scalar_boundary(u.boundary, u.dims, 'laplace')
    s_codes, s_val = _centered_rule(u, 'laplace')
    src = u.values.contiguous()
    folded = src.reshape(-1, *src.shape[-u.spatial_rank:])      # a centred vector field: the (B * C, *res) view
    meta = dict(be=be, grid=_cell_grid(u, folded.shape[0]), s_codes=s_codes, s_val=s_val, weights=w)
    if autodiff.needs_grad(folded):
        out = autodiff.LaplaceCentered.apply(meta, folded)
    else:
        out = be.empty(tuple(folded.shape), u.dtype)
        be.ctx.field_laplace_centered(meta['grid'], folded.data_ptr(), s_codes, s_val, w, out.data_ptr(), False, be.stream())
    return Field(u.resolution, u.bounds, u.boundary, out.reshape(src.shape), False, be, u.batched, vector=u.is_vector)


def _gradient_centered(s: Field, boundary) -> Field:
    """ g_d = (S[i + e_d] - S[i - e_d]) / (2 dx_d), S padded with the scalar's extrapolation -> centred vector field """
    from . import autodiff
    _check_diff_rank(s, "spatial_gradient(at='center')")
    ext = as_extrapolation(boundary) if boundary is not None else s.boundary.spatial_gradient()
    be = s.backend
    s_codes, s_val = _centered_rule(s, 'spatial_gradient')
    src = s.values.contiguous()
    meta = dict(be=be, grid=_cell_grid(s), s_codes=s_codes, s_val=s_val, rank=s.spatial_rank)
    if autodiff.needs_grad(src):
        out = autodiff.GradientCentered.apply(meta, src)
    else:
        out = be.empty((s.batch_size, s.spatial_rank) + tuple(s.resolution.values()), s.dtype)
        be.ctx.gradient_centered(meta['grid'], src.data_ptr(), s_codes, s_val, out.data_ptr(), be.stream())
    return Field(s.resolution, s.bounds, ext, out, False, be, s.batched, vector=True)


def _divergence_centered(v: Field) -> Field:
    """ sum_d (V_d[i + e_d] - V_d[i - e_d]) / (2 dx_d), every component padded with the field's extrapolation -> centred scalar """
    from . import autodiff
    _check_diff_rank(v, 'divergence')
    be = v.backend
    s_codes, s_val = _centered_rule(v, 'divergence')
    src = v.values.contiguous()
    meta = dict(be=be, grid=_cell_grid(v), s_codes=s_codes, s_val=s_val)
    if autodiff.needs_grad(src):
        out = autodiff.DivergenceCentered.apply(meta, src)
    else:
        out = be.empty((v.batch_size,) + tuple(v.resolution.values()), v.dtype)
        be.ctx.divergence_centered(meta['grid'], src.data_ptr(), s_codes, s_val, out.data_ptr(), be.stream())
    return Field(v.resolution, v.bounds, _difference_extrapolation(v.boundary, v.dims), out, False, be, v.batched)


def curl(v: Field, at: str = 'corner') -> Field:
    """ `field.curl(v, at='corner')` of a 2-D vector field (phi/field/_field_math.py:642-673): sampled at the (nx + 1) x (ny + 1) cell corners and
    returned as the CenteredGrid whose cell centres are the corners (resolution n + 1, bounds grown by dx / 2), extrapolation
    `v.boundary.spatial_gradient()`.
    Staggered: (vy[i, j] - vy[i - 1, j]) / dx - (vx[i, j] - vx[i, j - 1]) / dy on all n + 1 faces per axis, vx padded along y and vy along x. As in
    the reference, vx is padded with the boundary's y COMPONENT and vy with its x component (:655-656) -- the other component of a vector-valued
    constant; no difference for scalar-valued boundaries.
    Centred: (vx - vy)[ll] - (vx + vy)[ul] + (vx + vy)[lr] - (vx - vy)[ur] over the four cells around the corner, WITHOUT the factors 1 / dx and
    1 / 2 (as the reference): on square cells 2 dx times the staggered form. 3-D fields and other locations are not implemented. """
    from . import autodiff
    require_plain(v, 'curl')
    if not (v.is_staggered or v.is_vector):
        raise ValueError(f"curl requires a vector field but got {v!r}")
    if v.spatial_rank != 2 or at != 'corner':
        raise NotImplementedError("HIP backend: curl is implemented for 2-D vector fields at='corner' only")
    be = v.backend
    x, y = v.dims
    dx = v.dx
    res = {d: n + 1 for d, n in v.resolution.items()}
    bounds = Box(**{d: (lo - 0.5 * h, up + 0.5 * h) for d, lo, up, h in zip(v.dims, v.bounds.lower, v.bounds.upper, dx)})
    codes, vals = resolve(v.boundary, v.dims)
    grid = _cell_grid(v)
    shape = (v.batch_size, res[x], res[y])
    if v.is_staggered:
        baked = v.with_boundary(BOUNDARY)        # all n + 1 faces per axis, the missing ones from the field's own rule
        vx, vy = [t.contiguous() for t in baked.values]
        # vy is padded along x with the constant's x component, vx along y with its y component (the reference's literal choice)
        s_val = [[vals[0][s][0] for s in range(2)], [vals[1][s][1] for s in range(2)]]
        meta = dict(be=be, grid=grid, staggered=True, s_codes=codes, s_val=s_val, shape=shape)
        if autodiff.needs_grad(vx, vy):
            out = autodiff.Curl2D.apply(meta, vx, vy)
        else:
            out = be.empty(shape, v.dtype)
            be.ctx.curl_2d(grid, True, vx.data_ptr(), vy.data_ptr(), codes, s_val, out.data_ptr(), be.stream())
    else:
        s_codes, s_val = _centered_rule(v, 'curl')
        src = v.values.contiguous()
        meta = dict(be=be, grid=grid, staggered=False, s_codes=s_codes, s_val=s_val, shape=shape)
        if autodiff.needs_grad(src):
            out = autodiff.Curl2D.apply(meta, src)
        else:
            out = be.empty(shape, v.dtype)
            be.ctx.curl_2d(grid, False, src.data_ptr(), 0, s_codes, s_val, out.data_ptr(), be.stream())
    return Field(res, bounds, v.boundary.spatial_gradient(), out, False, be, v.batched)


def where(mask, a, b) -> Field:
    """ `field.where(mask_or_geometry, a, b)` on one grid (phi/field/_field_math.py:997-1015): `a` where the mask is non-zero, else `b`. A
    Geometry is rasterised to a hard mask on the grid of the first Field among a, b; numbers broadcast. """
    proto = next((f for f in (a, b, mask) if isinstance(f, Field)), None)
    if proto is None:
        raise ValueError("where: at least one of the arguments must be a Field")
    require_plain(proto, 'where')
    if isinstance(mask, Geometry):
        mask = resample(mask, to=proto)

    def vals(f):
        if not isinstance(f, Field):
            return [f] * proto.spatial_rank if proto.is_staggered else f
        require_plain(f, 'where')
        assert f.is_staggered == proto.is_staggered and same_grid(f, proto), f"where: fields on different sample points: {f!r} vs {proto!r}"
        if f.is_vector != proto.is_vector:      # a centred scalar against a centred vector: broadcast over the components
            return f.values.unsqueeze(1) if proto.is_vector else f.values
        return f.values
    m, va, vb = vals(mask), vals(a), vals(b)

    def pick(mm, xa, xb):
        cond = mm != 0 if isinstance(mm, torch.Tensor) else torch.as_tensor(bool(mm), device=proto.backend.device)
        xa = xa if isinstance(xa, torch.Tensor) else torch.as_tensor(float(xa), dtype=proto.dtype, device=proto.backend.device)
        xb = xb if isinstance(xb, torch.Tensor) else torch.as_tensor(float(xb), dtype=proto.dtype, device=proto.backend.device)
        return torch.where(cond, xa, xb)
    out = [pick(mm, xa, xb) for mm, xa, xb in zip(m, va, vb)] if proto.is_staggered else pick(m, va, vb)
    batched = any(isinstance(f, Field) and f.batched for f in (mask, a, b))
    return Field(proto.resolution, proto.bounds, proto.boundary, out, proto.is_staggered, proto.backend, batched, vector=proto.is_vector)


def mean(field: Field):
    """ `field.mean`: mean over the spatial dims per batch entry (phi/field/_field_math.py:780-796) """
    require_plain(field, 'mean')
    if field.is_staggered:
        raise NotImplementedError
    if field.is_vector:     # one value per component: (batch, D), or (D,) when not batched
        m = field.values.reshape(field.batch_size, field.spatial_rank, -1).mean(dim=2)
        return m if field.batched else m[0]
    m = field.values.reshape(field.batch_size, -1).mean(dim=1)
    return m if field.batched else m[0]


def resample(value, to: Field, soft: bool = False, balance: float = 0.5) -> Field:
    """ `resample(value, to=target)` / `value @ target` (phi/field/_resample.py:13-63). Implemented: same sample points (boundary
    change only), centred scalar [x constant vector] -> staggered faces on the same grid (sample_grid_at_faces,
    phi/field/_resample.py:272-276: mean of the two adjacent cells, padded with the scalar's extrapolation) as one HIP kernel
    per component (`phihip_centered_to_staggered`), and a `Geometry` -> mask on the target's sample points (set-up work, evaluated on
    the host): hard `lies_inside` or, with `soft=True`, `clip(balance - sdf / cell_radius, 0, 1)`
    (`resample(Sphere(...), to=smoke, soft=True)`, Smoke_Plume.ipynb cell 3; phi/field/_resample.py:192-210, phi/geom/_geom.py:278-308). """
    if isinstance(value, Geometry):
        radius = float(np.sqrt(sum((0.5 * h) ** 2 for h in to.dx)))

        def mask(pts):
            if soft:
                return np.clip(balance - value.approximate_signed_distance(pts) / radius, 0, 1)
            return value.lies_inside(pts).astype(np.float64)
        if to.is_staggered:
            comps = [_tensor_from(mask(_sample_points(to.resolution, to.bounds, d, to.boundary)), component_shape(to.resolution, to.boundary, d),
                                  to.backend, to.dtype) for d in range(to.spatial_rank)]
            B = max(t.shape[0] for t, _ in comps)
            return Field(to.resolution, to.bounds, to.boundary, [t if t.shape[0] == B else t.expand(B, *t.shape[1:]).contiguous() for t, _ in comps],
                         True, to.backend, any(b for _, b in comps))
        t, batched = _tensor_from(mask(_sample_points(to.resolution, to.bounds, None, to.boundary)), tuple(to.resolution.values()), to.backend, to.dtype)
        return Field(to.resolution, to.bounds, to.boundary, t, False, to.backend, batched)
    if value.is_staggered == to.is_staggered and same_grid(value, to) and value.vector_scale is None:
        if value.is_staggered and value.boundary != to.boundary:
            return value.with_boundary(to.boundary)
        return Field(value.resolution, value.bounds, to.boundary, value.values, value.is_staggered, value.backend, value.batched, vector=value.is_vector)
    if value.vector_scale is not None and to.is_vector:       # `(s * vec) @ centred_vector_target`: a real centred vector field
        if not same_grid(value, to):
            from . import sampling
            return sampling.resample_general(value, to)
        w = torch.as_tensor(value.vector_scale, dtype=value.dtype, device=value.backend.device).reshape(1, -1, *([1] * value.spatial_rank))
        return Field(to.resolution, to.bounds, to.boundary, value.values.unsqueeze(1) * w, False, value.backend, value.batched, vector=True)
    if (value.is_vector and to.is_staggered) or (value.is_staggered and to.is_centered):
        return _resample_vector(value, to)
    if value.vector_scale is not None and to.is_centered:
        raise NotImplementedError("HIP backend: a `scalar * vector` field can only be resampled to a StaggeredGrid (centred vector fields "
                                  "are not implemented)")
    if value.is_centered and to.is_staggered and same_grid(value, to):
        be = value.backend
        scale = value.vector_scale or [1.0] * value.spatial_rank
        B = max(value.batch_size, to.batch_size)
        src = value.values if value.batch_size == B else value.values.expand(B, *value.values.shape[1:])
        src = src.contiguous()
        proto = Field(to.resolution, to.bounds, to.boundary, None, True, be, False)
        grid = _capi.make_grid(value.spatial_rank, _torch_dtype_code(value.dtype), B, list(to.resolution.values()), to.bounds.lower,
                               to.bounds.upper, proto._codes, proto._bc_val)
        comps = [be.empty((B,) + component_shape(to.resolution, to.boundary, d), value.dtype) for d in range(value.spatial_rank)]
        s_codes, s_vals = resolve(value.boundary, value.dims)
        s_val = [[s_vals[a][s][0] if isinstance(value.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)]
                 for a, d in enumerate(value.dims)]
        from . import autodiff
        if autodiff.needs_grad(src):
            meta = dict(be=be, grid=grid, s_codes=s_codes, s_val=s_val, vector=scale, shapes=[tuple(c.shape) for c in comps], dtype=value.dtype)
            comps = list(autodiff.CenteredToStaggered.apply(meta, src))
        else:
            be.ctx.centered_to_staggered(grid, src.data_ptr(), s_codes, s_val, scale, False, _ptrs(comps), be.stream())
        return Field(to.resolution, to.bounds, to.boundary, comps, True, be, value.batched or to.batched)
    from . import sampling
    return sampling.resample_general(value, to)     # different grids: one gather per (component of the) target


def _centered_rule(field: Field, what: str):
    """ (codes[D][2], consts[D][2]) of a centred field's extrapolation, shared by the components of a centred vector field """
    require_scalar_boundary(field.boundary, field.dims, what)
    codes, vals = resolve(field.boundary, field.dims)
    consts = [[vals[a][s][0] if isinstance(field.boundary.side(d, bool(s)), ConstantExtrapolation) else 0.0 for s in range(2)]
              for a, d in enumerate(field.dims)]
    return codes, consts


def _same_periodicity(a: Extrapolation, b: Extrapolation, dims) -> bool:
    ca, cb = resolve(a, dims)[0], resolve(b, dims)[0]
    return all((x == _capi.BC_PERIODIC) == (y == _capi.BC_PERIODIC) for pa, pb in zip(ca, cb) for x, y in zip(pa, pb))


def _resample_vector(value: Field, to: Field) -> Field:
    """ staggered -> cell centres (`at_centers`, phihip_staggered_to_centered) and centred vector -> stored faces
    (phihip_centered_vector_to_staggered) on the same grid, one launch each; other grids and inputs that require grad take the general
    sampling path (differentiable through GridSample) """
    from . import autodiff, sampling
    if value.spatial_rank not in (2, 3):
        raise NotImplementedError(f"HIP backend: centred vector fields on {value.spatial_rank}-D grids are not implemented (2-D and 3-D only)")
    src = value.values if value.is_staggered else [value.values]
    # the face kernel pads with the centred field's own rule, so it needs the target's periodicity; otherwise (and on other grids, or with
    # gradients) the general gather samples the field at the target's points with its extrapolation -- the same values
    if not same_grid(value, to) or autodiff.needs_grad(*src) or (value.is_vector and not _same_periodicity(value.boundary, to.boundary, value.dims)):
        return sampling.resample_general(value, to)
    be = value.backend
    B = value.batch_size
    if value.is_staggered:          # -> centres: the velocity's own rule fills the faces that are not stored
        vel = [t.contiguous() for t in value.values]
        out = be.empty((B, value.spatial_rank) + tuple(value.resolution.values()), value.dtype)
        be.ctx.staggered_to_centered(value.grid_struct(), _ptrs(vel), out.data_ptr(), be.stream())
        return Field(to.resolution, to.bounds, to.boundary, out, False, be, value.batched, vector=True)
    s_codes, s_val = _centered_rule(value, 'resample (centred vector -> faces)')
    proto = Field(to.resolution, to.bounds, to.boundary, None, True, be, False)
    grid = _capi.make_grid(value.spatial_rank, _torch_dtype_code(value.dtype), B, list(to.resolution.values()), to.bounds.lower,
                           to.bounds.upper, proto._codes, proto._bc_val)
    comps = [be.empty((B,) + component_shape(to.resolution, to.boundary, d), value.dtype) for d in range(value.spatial_rank)]
    src = value.values.contiguous()
    be.ctx.centered_vector_to_staggered(grid, src.data_ptr(), B, s_codes, s_val, _ptrs(comps), be.stream())
    return Field(to.resolution, to.bounds, to.boundary, comps, True, be, value.batched)


def vector_scaled(s: Field, vector: Sequence[float]) -> Field:
    """ `smoke * (0, 0.1)`: a centred scalar times a constant vector, kept lazily until it is resampled with `@`. """
    assert s.is_centered and len(vector) == s.spatial_rank
    vec = [float(c) for c in vector]
    if s.vector_scale is not None:             # (s * (0, 1)) * (2, 3): component-wise product of the vectors
        vec = [a * b for a, b in zip(s.vector_scale, vec)]
    return Field(s.resolution, s.bounds, s.boundary, s.values, False, s.backend, s.batched, vec)


def assert_close(*fields, rel_tolerance: float = 1e-5, abs_tolerance: float = 0, msg: str = ""):
    """ `field.assert_close` (values only) """
    ref = fields[0]
    ref_np = ref.numpy() if isinstance(ref, Field) else ref
    for other in fields[1:]:
        oth_np = other.numpy() if isinstance(other, Field) else other
        pairs = zip(ref_np, oth_np) if isinstance(ref_np, list) else [(ref_np, oth_np)]
        for a, b in pairs:
            np.testing.assert_allclose(np.asarray(b), np.asarray(a), rtol=rel_tolerance, atol=abs_tolerance, err_msg=msg)

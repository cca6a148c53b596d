"""
ctypes binding of ``libphihip.so``. ``include/phihip.h`` is the single declaration of the C ABI: the exported names, every parameter
list and every integer constant of this module are read from it at import (`load_header`). Written by hand are only the five
structures and the wrapper methods of `Context`; tests/test_capi_symbols.py checks both against the header.

This is the only place the package touches native code. There is **no CPU fallback**: if the shared library is
missing `load_default_library()` raises `PhiHipLibraryError`, and creating a context without a HIP device fails with
``PHIHIP_ERR_NO_DEVICE``.
"""
import ctypes
import os
import re
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int32, c_int64, c_longlong, c_size_t, c_void_p
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(_HERE, "..", "include", "phihip.h")


class PhiHipError(RuntimeError):
    """ A libphihip call returned a negative status. """

    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class PhiHipLibraryError(ImportError):
    """ libphihip.so could not be loaded (not built, or ROCm runtime missing), or include/phihip.h declares what this binding cannot express. """


class Grid(ctypes.Structure):
    """ mirrors ``phihip_grid`` """
    _fields_ = [("rank", c_int32), ("dtype", c_int32), ("batch", c_int32), ("res", c_int32 * 3),
                ("lower", c_double * 3), ("upper", c_double * 3), ("bc", (c_int32 * 2) * 3),
                ("bc_val", ((c_double * 3) * 2) * 3)]


class ObstacleStruct(ctypes.Structure):
    """ phihip_obstacle """
    _fields_ = [("kind", c_int32), ("group", c_int32), ("embed_mask", c_int32), ("reserved", c_int32), ("center", c_double * 3), ("half_size", c_double * 3),
                ("velocity", c_double * 3), ("angular_velocity", c_double * 3), ("rotation", c_double * 9)]


class SdfGridStruct(ctypes.Structure):
    """ phihip_sdf_grid """
    _fields_ = [("sdf", c_void_p), ("dtype", c_int32), ("rank", c_int32), ("res", c_int32 * 3), ("approximate_outside", c_int32), ("lower", c_double * 3),
                ("upper", c_double * 3), ("center", c_double * 3), ("bounding_radius", c_double)]


class Solve(ctypes.Structure):
    """ mirrors ``phihip_solve`` """
    _fields_ = [("rel_tol", c_double), ("abs_tol", c_double), ("max_iterations", c_int32), ("refresh_every", c_int32),
                ("check_every", c_int32), ("method", c_int32)]


class SolveInfo(ctypes.Structure):
    """ mirrors ``phihip_solve_info`` """
    _fields_ = [("residual_sq", c_double), ("rhs_sq", c_double), ("iterations", c_int32), ("converged", c_int32),
                ("diverged", c_int32), ("reserved", c_int32)]


_Ptr3, _Vec3, _Bc, _Val = c_void_p * 3, c_double * 3, (c_int32 * 2) * 3, (c_double * 2) * 3

# ---- the header as the declaration: every spelling a return value or a parameter of include/phihip.h may have (declaration without `const`, name
#      and spaces), plus 1-D arrays `int32_t[N]` / `double[N]`. Device pointers and the context handle stay c_void_p: callers pass plain ints. ----
_RETURNS = {"int": c_int, "const char*": c_char_p}
_PARAMETERS = {
    "int": c_int, "int32_t": c_int32, "int64_t": c_int64, "long long": c_longlong, "double": c_double,
    "void*": c_void_p, "uint8_t*": c_void_p, "double*": c_void_p, "phihip_ctx*": c_void_p, "phihip_ctx**": POINTER(c_void_p),
    "int32_t*": POINTER(c_int32), "size_t*": POINTER(c_size_t), "phihip_grid*": POINTER(Grid), "phihip_solve*": POINTER(Solve),
    "phihip_solve_info*": POINTER(SolveInfo), "phihip_obstacle*": POINTER(ObstacleStruct), "phihip_sdf_grid*": POINTER(SdfGridStruct),
    "void*[3]": POINTER(_Ptr3), "int32_t[3][2]": POINTER(_Bc), "double[3][2]": POINTER(_Val),
}


def load_header(text: str):
    """ ({name: (restype, argtypes)} of every prototype, {PHIHIP_X: n} of every enum value and integer #define) of a phihip.h text.
    A spelling that `_RETURNS` / `_PARAMETERS` do not list raises `PhiHipLibraryError`: nothing is guessed. """
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {name: int(n) for name, n in re.findall(r"#define[ \t]+(PHIHIP_\w+)[ \t]+(-?\d+)", text)      # integer #defines ...
                 + re.findall(r"(PHIHIP_\w+)\s*=\s*(-?\d+)", text)}                                            # ... and enum values

    def ctype(table, spelling, name, decl):
        array = re.fullmatch(r"(int32_t|double)\[(\d+)\]", spelling)
        if array:
            return POINTER(table[array[1]] * int(array[2]))
        if spelling not in table:
            raise PhiHipLibraryError(f"include/phihip.h: {name}: no ctypes mapping for the spelling '{spelling}' of '{decl}'")
        return table[spelling]

    signatures = {}
    for ret, name, params in re.findall(r"^([\w \*]+?)\s*\b(phihip_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        argtypes = []
        for decl in [" ".join(p.split()) for p in params.split(",") if p.strip() != "void"]:
            base, bounds = re.fullmatch(r"(.*?)\w+((?:\[\w+\])*)", decl).groups()
            bounds = re.sub(r"PHIHIP_\w+", lambda m: str(constants.get(m[0], m[0])), bounds)
            argtypes.append(ctype(_PARAMETERS, " ".join(re.sub(r"\bconst\b", " ", base).split()).replace(" *", "*") + bounds, name, decl))
        signatures[name] = (ctype(_RETURNS, ret.strip(), name, ret.strip()), argtypes)
    return signatures, constants


with open(HEADER_PATH) as _header:
    SIGNATURES, CONSTANTS = load_header(_header.read())
EXPORTED_SYMBOLS = tuple(SIGNATURES)

VERSION = CONSTANTS["PHIHIP_VERSION"]
PHIHIP_F32, PHIHIP_F64 = CONSTANTS["PHIHIP_F32"], CONSTANTS["PHIHIP_F64"]
BC_PERIODIC, BC_CLOSED, BC_OPEN = (CONSTANTS["PHIHIP_BC_" + k] for k in ("PERIODIC", "CLOSED", "OPEN"))
OBSTACLE_BOX, OBSTACLE_SPHERE, OBSTACLE_SDF, OBSTACLE_CYLINDER = (CONSTANTS["PHIHIP_OBSTACLE_" + k] for k in ("BOX", "SPHERE", "SDF", "CYLINDER"))
SDF_SLOTS = CONSTANTS["PHIHIP_SDF_SLOTS"]
DIV_BALANCE, DIV_FINITE_GUARD = CONSTANTS["PHIHIP_DIV_BALANCE"], CONSTANTS["PHIHIP_DIV_FINITE_GUARD"]      # bits of the `balance` argument
_K = {k[len("PHIHIP_K_"):].lower(): n for k, n in CONSTANTS.items() if k.startswith("PHIHIP_K_")}      # enum phihip_kernel_id
K_COUNT = _K.pop("count")
K_NAMES = tuple(sorted(_K, key=_K.get))
STATUS_NAMES = {n: k for k, n in CONSTANTS.items() if k == "PHIHIP_OK" or k.startswith("PHIHIP_ERR_")}      # enum phihip_status


def make_sdf_grid(ptr: int, dtype: int, res, lower, upper, center, bounding_radius: float, approximate_outside: bool) -> SdfGridStruct:
    """ values at `ptr` (device, dense, last axis fast) of resolution `res` on the box [lower, upper], all in the order of the grids the obstacle meets """
    d = SdfGridStruct()
    d.sdf, d.dtype, d.rank, d.approximate_outside, d.bounding_radius = ptr or None, int(dtype), len(res), int(bool(approximate_outside)), float(bounding_radius)
    for k in range(len(res)):
        d.res[k], d.lower[k], d.upper[k], d.center[k] = int(res[k]), float(lower[k]), float(upper[k]), float(center[k])
    return d


def make_obstacles(items) -> "ctypes.Array":
    """ items: sequence of dicts(kind, center, half_size, velocity, angular_velocity[, rotation, group]) -> ctypes array of phihip_obstacle """
    arr = (ObstacleStruct * max(1, len(items)))()
    for k, it in enumerate(items):
        arr[k].kind = int(it["kind"])
        arr[k].group = int(it.get("group", 0))
        arr[k].embed_mask = int(it.get("embed_mask", 0))
        arr[k].reserved = int(it.get("slot", it.get("axis", 0)))      # kind OBSTACLE_SDF: the slot of Context.sdf_bind; OBSTACLE_CYLINDER: the axis index
        for d, val in enumerate(it.get("center", ())):
            arr[k].center[d] = float(val)
        for d, val in enumerate(it.get("half_size", ())):
            arr[k].half_size[d] = float(val)
        for d, val in enumerate(it.get("velocity", ())):
            arr[k].velocity[d] = float(val)
        for d, val in enumerate(it.get("angular_velocity", ())):
            arr[k].angular_velocity[d] = float(val)
        rot = it.get("rotation")
        if rot is not None:   # (rank x rank) matrix, box frame -> world
            for a, row in enumerate(rot):
                for c, val in enumerate(row):
                    arr[k].rotation[3 * a + c] = float(val)
    return arr


def make_grid(rank: int, dtype: int, batch: int, res, lower, upper, bc, bc_val=None) -> Grid:
    g = Grid()
    g.rank, g.dtype, g.batch = int(rank), int(dtype), int(batch)
    for d in range(rank):
        g.res[d] = int(res[d])
        g.lower[d] = float(lower[d])
        g.upper[d] = float(upper[d])
        for s in range(2):
            g.bc[d][s] = int(bc[d][s])
            for c in range(rank):
                g.bc_val[d][s][c] = float(bc_val[d][s][c]) if bc_val is not None else 0.0
    return g


class _Missing:
    """ inert stand-in of a symbol that a strict=False library lacks: not callable """
    argtypes = restype = None


class Library:
    """ typed function table of one loaded libphihip """

    def __init__(self, path: str, strict: bool = True):
        """ strict=False (benchmark A/B of an older build only): symbols missing from the library are skipped """
        self.path = os.path.abspath(path)
        # PyTorch-ROCm ships its own libamdhip64: whichever HIP runtime is loaded first owns the devices, a second copy sees "No HIP
        # GPUs". When torch is installed (it provides the device tensors for the Python layer), let it load its runtime first so that
        # libphihip binds to the same one. C / C++ callers of the ABI are not affected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            self.dll = ctypes.CDLL(self.path)
        except OSError as exc:
            raise PhiHipLibraryError(f"cannot load {self.path}: {exc}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                     f"(hipcc --offload-arch=gfx950); there is no CPU fallback.") from exc
        missing = [s for s in EXPORTED_SYMBOLS if not hasattr(self.dll, s)]
        if missing and strict:
            raise PhiHipLibraryError(f"{self.path} lacks symbols declared in include/phihip.h: {missing}")
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in missing:
                setattr(self.dll, name, _Missing())
            else:
                fn = getattr(self.dll, name)
                fn.restype, fn.argtypes = restype, argtypes

    def check(self, status: int):
        if status != 0:
            raise PhiHipError(status, (self.dll.phihip_last_error() or b"").decode(errors="replace"))

    def version(self) -> int:
        return self.dll.phihip_version()

    def build_id(self) -> str:
        """ "<git commit>[+dirty] src:<hash of the sources the library was compiled from>" (phihip_build_id) """
        fn = getattr(self.dll, "phihip_build_id", None)
        raw = fn() if callable(fn) else None
        return (raw or b"unknown src:unknown").decode(errors="replace")

    def built_from_tree(self) -> bool:
        """ the library was compiled from the kernel sources that sit next to it now (stale-.so check: the .so is not in git) """
        return self.build_id().rsplit("src:", 1)[-1] == source_hash()


def source_hash() -> str:
    """ sha1 (16 hex digits) over csrc/*.hip, csrc/*.hpp in name order and include/phihip.h -- the Makefile embeds the same value """
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")))
    h = hashlib.sha1()
    for f in [os.path.join(csrc, f) for f in files] + [HEADER_PATH]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _ref3(ptrs: Optional[Sequence[int]]):
    """ `T* const x[3]`: up to three device pointers by reference (0 and unused trailing entries NULL), or NULL for None (an optional array) """
    return None if ptrs is None else byref(_Ptr3(*ptrs))


def _vec3(values):
    """ `const double x[3]`: the values, zero-padded, by reference """
    return byref(_Vec3(*[float(x) for x in values]))


def _scalar_bc(grid, s_bc, s_val):
    """ `s_bc[3][2], s_val[3][2]` by reference: the extrapolation of a centred field on the axes of `grid`; s_val None = zeros """
    bc, val = _Bc(), _Val()
    for d in range(grid.rank):
        for side in range(2):
            bc[d][side] = int(s_bc[d][side])
            val[d][side] = float(s_val[d][side]) if s_val is not None else 0.0
    return byref(bc), byref(val)


class Context:
    """ owns one ``phihip_ctx`` (device + workspace). Not thread-safe; one per (process, device). """

    def __init__(self, lib: Library, device: int = 0):
        self.lib, self._dll, self._check = lib, lib.dll, lib.check
        self.handle = c_void_p()
        self._check(self._dll.phihip_ctx_create(int(device), byref(self.handle)))

    def close(self):
        if self.handle:
            self._dll.phihip_ctx_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thin typed wrappers (pointers are plain ints; `x or None`: 0 is NULL) ----
    def component_shape(self, grid: Grid, comp: int):
        out = (c_int32 * 3)()
        self._check(self._dll.phihip_component_shape(byref(grid), comp, byref(out)))      # (the one entry point without a context)
        return tuple(out[d] for d in range(grid.rank))

    def advect_staggered(self, grid, field, velocity, out, dt, stream=0):
        self._check(self._dll.phihip_advect_staggered(self.handle, byref(grid), _ref3(field), _ref3(velocity), _ref3(out), float(dt), stream or None))

    def advect_centered(self, grid, s, s_bc, s_val, velocity, out, dt, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_advect_centered(self.handle, byref(grid), s, bc, val, _ref3(velocity), out, float(dt), stream or None))

    def advect_centered_vector(self, grid, field, field_batch, components, s_bc, s_val, velocity, velocity_batch, out, dt, stream=0):
        """ centred field (field_batch, components, *res) advected by a centred velocity (velocity_batch, rank, *res) on the same grid """
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_advect_centered_vector(self.handle, byref(grid), field, int(field_batch), int(components), bc, val, velocity,
            int(velocity_batch), out, float(dt), stream or None))

    def staggered_to_centered(self, grid, velocity, out, stream=0):
        """ staggered components -> cell centres, out (batch, rank, *res) """
        self._check(self._dll.phihip_staggered_to_centered(self.handle, byref(grid), _ref3(velocity), out, stream or None))

    def centered_vector_to_staggered(self, grid, field, field_batch, s_bc, s_val, out, stream=0):
        """ centred vector (field_batch, rank, *res) -> the stored faces of `grid` """
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_centered_vector_to_staggered(self.handle, byref(grid), field, int(field_batch), bc, val, _ref3(out),
            stream or None))

    def grid_sample(self, grid, values, values_batch, coords, points, out, out_min=0, out_max=0, stream=0):
        """ math.grid_sample: `grid` describes the VALUES array (res = its shape, bc / bc_val[..][0] = its extrapolation) """
        self._check(self._dll.phihip_grid_sample(self.handle, byref(grid), values, int(values_batch), _ref3(coords), int(points), out or None,
            out_min or None, out_max or None, stream or None))

    def grid_sample_backward(self, grid, values, values_batch, coords, points, grad_out, grad_values, grad_coords, stream=0):
        self._check(self._dll.phihip_grid_sample_backward(self.handle, byref(grid), values, int(values_batch), _ref3(coords), int(points), grad_out,
            grad_values or None, _ref3(grad_coords), stream or None))

    def mac_cormack_staggered(self, grid, field, velocity, out, dt, correction_strength=1.0, stream=0):
        self._check(self._dll.phihip_mac_cormack_staggered(self.handle, byref(grid), _ref3(field), _ref3(velocity), _ref3(out), float(dt),
            float(correction_strength), stream or None))

    def mac_cormack_centered(self, grid, s, s_bc, s_val, velocity, out, dt, correction_strength=1.0, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_mac_cormack_centered(self.handle, byref(grid), s, bc, val, _ref3(velocity), out, float(dt),
            float(correction_strength), stream or None))

    def centered_to_staggered(self, grid, s, s_bc, s_val, vector, accumulate, out, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_centered_to_staggered(self.handle, byref(grid), s, bc, val, _vec3(vector), int(bool(accumulate)), _ref3(out),
            stream or None))

    def advect_staggered_backward(self, grid, field, velocity, grad_out, dt, grad_field, grad_velocity, stream=0):
        self._check(self._dll.phihip_advect_staggered_backward(self.handle, byref(grid), _ref3(field), _ref3(velocity), _ref3(grad_out), float(dt),
            _ref3(grad_field), _ref3(grad_velocity), stream or None))

    def advect_centered_backward(self, grid, s, s_bc, s_val, velocity, grad_out, dt, grad_s, grad_velocity, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_advect_centered_backward(self.handle, byref(grid), s, bc, val, _ref3(velocity), grad_out, float(dt),
            grad_s or None, _ref3(grad_velocity), stream or None))

    def mac_cormack_staggered_backward(self, grid, field, velocity, grad_out, dt, strength, grad_field, grad_velocity, stream=0):
        self._check(self._dll.phihip_mac_cormack_staggered_backward(self.handle, byref(grid), _ref3(field), _ref3(velocity), _ref3(grad_out),
            float(dt), float(strength), _ref3(grad_field), _ref3(grad_velocity), stream or None))

    def mac_cormack_centered_backward(self, grid, s, s_bc, s_val, velocity, grad_out, dt, strength, grad_s, grad_velocity, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_mac_cormack_centered_backward(self.handle, byref(grid), s, bc, val, _ref3(velocity), grad_out, float(dt),
            float(strength), grad_s, _ref3(grad_velocity), stream or None))

    def diffuse_explicit_backward(self, grid, grad_out, grad_in, diffusivity_dt, stream=0):
        self._check(self._dll.phihip_diffuse_explicit_backward(self.handle, byref(grid), _ref3(grad_out), _ref3(grad_in), float(diffusivity_dt),
            stream or None))

    def diffuse_explicit_centered(self, grid, s, s_bc, s_val, out, diffusivity_dt, adjoint=False, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_diffuse_explicit_centered(self.handle, byref(grid), s, bc, val, out, float(diffusivity_dt), int(bool(adjoint)),
            stream or None))

    def centered_to_staggered_backward(self, grid, s_bc, vector, grad_out, grad_s, stream=0):
        bc, _ = _scalar_bc(grid, s_bc, None)
        self._check(self._dll.phihip_centered_to_staggered_backward(self.handle, byref(grid), bc, _vec3(vector), _ref3(grad_out), grad_s,
            stream or None))

    def make_incompressible_backward(self, grid, flags, mask_batch, balance, grad_velocity, grad_pressure, solve: Solve, want_info=True,
                                     stream=0):
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_make_incompressible_backward(self.handle, byref(grid), flags or None, int(mask_batch),
            int(balance) & DIV_BALANCE, _ref3(grad_velocity), grad_pressure or None, byref(solve), info, stream or None))
        return list(info) if want_info else None

    # ---- f4: slab-decomposed CG phases (see include/phihip.h) ----
    def slab_residual(self, grid, halo, flags, x, x_halo, rhs, r, sums, keep_going=False, stream=0):
        self._check(self._dll.phihip_slab_residual(self.handle, byref(grid), int(halo[0]), int(halo[1]), flags or None, x, x_halo[0] or None,
            x_halo[1] or None, rhs, r, sums, int(bool(keep_going)), stream or None))

    def slab_matvec(self, grid, halo, flags, first, sums_in, r, r_halo, d_old, d_halo, d_new, sum_out, solve: Solve, stream=0):
        self._check(self._dll.phihip_slab_matvec(self.handle, byref(grid), int(halo[0]), int(halo[1]), flags or None, int(bool(first)), sums_in, r,
            r_halo[0] or None, r_halo[1] or None, d_old, d_halo[0] or None, d_halo[1] or None, d_new, sum_out, byref(solve), stream or None))

    def slab_update(self, grid, halo, flags, sum_in, d, d_halo, x, r, sum_out, solve: Solve, x_only=False, stream=0):
        self._check(self._dll.phihip_slab_update(self.handle, byref(grid), int(halo[0]), int(halo[1]), flags or None, sum_in, d, d_halo[0] or None,
            d_halo[1] or None, x, r or None, sum_out or None, int(bool(x_only)), byref(solve), stream or None))

    def slab_state(self, grid, first, sums_in, solve: Solve, peek=False, stream=0):
        info = (SolveInfo * grid.batch)()
        self._check(self._dll.phihip_slab_state(self.handle, byref(grid), int(bool(first)), sums_in, byref(solve), info, int(bool(peek)),
            stream or None))
        return list(info)

    def obstacle_accessible(self, grid, obstacles, count, accessible, stream=0):
        self._check(self._dll.phihip_obstacle_accessible(self.handle, byref(grid), obstacles, int(count), accessible, stream or None))

    def apply_obstacles(self, grid, obstacles, count, velocity, stream=0):
        self._check(self._dll.phihip_apply_obstacles(self.handle, byref(grid), obstacles, int(count), _ref3(velocity), stream or None))

    def sdf_bind(self, desc: SdfGridStruct) -> int:
        """ binds a signed-distance grid to a free slot of this context; the array at desc.sdf must outlive the binding """
        slot = c_int32(-1)
        self._check(self._dll.phihip_sdf_bind(self.handle, byref(desc), byref(slot)))
        return int(slot.value)

    def sdf_release(self, slot: int):
        self._check(self._dll.phihip_sdf_release(self.handle, int(slot)))

    def sdf_from_analytic(self, desc: SdfGridStruct, obstacles, count, out, stream=0):
        """ sample_sdf: min over the analytic obstacles of the signed distance at the cell centres of `desc` -> out (device, desc.dtype) """
        self._check(self._dll.phihip_sdf_from_analytic(self.handle, byref(desc), obstacles, int(count), out, stream or None))

    def build_cellflags(self, grid, accessible, active, mask_batch, flags, stream=0):
        self._check(self._dll.phihip_build_cellflags(self.handle, byref(grid), accessible or None, active or None, int(mask_batch), flags,
            stream or None))

    def divergence(self, grid, velocity, flags, mask_batch, balance, div, stream=0):
        self._check(self._dll.phihip_divergence(self.handle, byref(grid), _ref3(velocity), flags or None, int(mask_batch), int(balance), div,
            stream or None))

    def laplace_apply(self, grid, flags, mask_batch, p, out, stream=0):
        self._check(self._dll.phihip_laplace_apply(self.handle, byref(grid), flags or None, int(mask_batch), p, out, stream or None))

    def cg_solve(self, grid, flags, mask_batch, rhs, x, solve: Solve, want_info=True, stream=0):
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_cg_solve(self.handle, byref(grid), flags or None, int(mask_batch), rhs, x, byref(solve), info, stream or None))
        return list(info) if want_info else None

    def precondition_apply(self, grid, flags, mask_batch, r, z, stream=0):
        """ one multigrid V-cycle z = M r (M ~ A^-1, the preconditioner of METHOD_CG_MULTIGRID); r and z must not alias """
        self._check(self._dll.phihip_precondition_apply(self.handle, byref(grid), flags or None, int(mask_batch), r, z, stream or None))

    def set_multigrid(self, sweeps: int = 0, coarsest_cells: int = 0, coarsest_sweeps: int = 0, omega: float = 0.0):
        """ parameters of the V-cycle; a value <= 0 keeps the current one (defaults 2, 4, 30, 0.8) """
        self._check(self._dll.phihip_set_multigrid(self.handle, int(sweeps), int(coarsest_cells), int(coarsest_sweeps), float(omega)))

    def query_multigrid(self) -> dict:
        """ levels and kernel launches of the most recent V-cycle on this context """
        out = (c_int32 * 2)()
        self._check(self._dll.phihip_query_multigrid(self.handle, byref(out)))
        return {"levels": int(out[0]), "launches": int(out[1])}

    def cg_solve_shifted(self, grid, identity, scale, rhs, x, solve: Solve, want_info=True, stream=0):
        """ CG on (identity * I + scale * L) x = rhs with the pressure operator L of `grid` (no obstacle flags) """
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_cg_solve_shifted(self.handle, byref(grid), float(identity), float(scale), rhs, x, byref(solve), info,
            stream or None))
        return list(info) if want_info else None

    def solve_residuals(self, batch, out_device, stream=0):
        """ device-side (||r||^2, ||rhs||^2) per batch entry of the last solve, no host sync """
        self._check(self._dll.phihip_solve_residuals(self.handle, int(batch), out_device, stream or None))

    def solve_relative_residual(self, batch, out_device, stream=0):
        """ device-side max over the batch entries of ||r|| / ||rhs|| of the last solve (one double), no host sync """
        self._check(self._dll.phihip_solve_relative_residual(self.handle, int(batch), out_device, stream or None))

    def grad_subtract(self, grid, flags, mask_batch, p, velocity, stream=0):
        self._check(self._dll.phihip_grad_subtract(self.handle, byref(grid), flags or None, int(mask_batch), p, _ref3(velocity), stream or None))

    def make_incompressible(self, grid, velocity, soft_mask, flags, mask_batch, balance, pressure, div_out, solve: Solve,
                            want_info=True, stream=0):
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_make_incompressible(self.handle, byref(grid), _ref3(velocity), _ref3(soft_mask), flags or None, int(mask_batch),
            int(balance), pressure, div_out or None, byref(solve), info, stream or None))
        return list(info) if want_info else None

    def diffuse_explicit(self, grid, velocity, out, diffusivity_dt, stream=0):
        self._check(self._dll.phihip_diffuse_explicit(self.handle, byref(grid), _ref3(velocity), _ref3(out), float(diffusivity_dt), stream or None))

    def diffuse_implicit(self, grid, velocity, out, diffusivity_dt, solve: Solve, stream=0, want_info=True):
        """ diffuse.implicit of a staggered field: (I - k dt L) out = velocity per component, CG from x0 = velocity; returns rank x batch SolveInfo
        (want_info=False: info = NULL, no host read-back -- the capture-safe form) """
        info = (SolveInfo * (grid.rank * grid.batch))() if want_info else None
        self._check(self._dll.phihip_diffuse_implicit(self.handle, byref(grid), _ref3(velocity), _ref3(out), float(diffusivity_dt), byref(solve),
            info, stream or None))
        return list(info) if want_info else None

    def diffuse_implicit_centered(self, grid, s, s_bc, s_val, out, diffusivity_dt, solve: Solve, stream=0, want_info=True):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_diffuse_implicit_centered(self.handle, byref(grid), s, bc, val, out, float(diffusivity_dt), byref(solve), info,
            stream or None))
        return list(info) if want_info else None

    def diffuse_explicit_centered_coef(self, grid, s, s_bc, s_val, coef, c_batch, c_bc, c_val, kdt, out, adjoint=False, stream=0):
        """ one substep of diffuse.explicit with a varying / per-axis diffusivity: out = s + L s (adjoint: out += (I + L)^T s);
        coef = 0 -> 1 everywhere; kdt = k_d * dt' per grid axis """
        bc, val = _scalar_bc(grid, s_bc, s_val)
        cbc, cval = _scalar_bc(grid, c_bc if coef else s_bc, c_val if coef else s_val)
        self._check(self._dll.phihip_diffuse_explicit_centered_coef(self.handle, byref(grid), s, bc, val, coef or None, int(c_batch), cbc, cval,
            _vec3(kdt), out, int(bool(adjoint)), stream or None))

    # --- grid differential operators (csrc/diffops.hpp); adjoint / *_backward accumulate the input gradient ---
    def field_laplace(self, grid, velocity, out, weight, adjoint=False, stream=0):
        self._check(self._dll.phihip_field_laplace(self.handle, byref(grid), _ref3(velocity), _ref3(out), float(weight), int(bool(adjoint)),
            stream or None))

    def field_laplace_centered(self, grid, s, s_bc, s_val, weights, out, adjoint=False, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_field_laplace_centered(self.handle, byref(grid), s, bc, val, _vec3(weights), out, int(bool(adjoint)),
            stream or None))

    def gradient_centered(self, grid, s, s_bc, s_val, out, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_gradient_centered(self.handle, byref(grid), s, bc, val, out, stream or None))

    def gradient_centered_backward(self, grid, s_bc, grad_out, grad_s, stream=0):
        bc, _ = _scalar_bc(grid, s_bc, None)
        self._check(self._dll.phihip_gradient_centered_backward(self.handle, byref(grid), bc, grad_out, grad_s, stream or None))

    def divergence_centered(self, grid, field, s_bc, s_val, out, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_divergence_centered(self.handle, byref(grid), field, bc, val, out, stream or None))

    def divergence_centered_backward(self, grid, s_bc, grad_out, grad_field, stream=0):
        bc, _ = _scalar_bc(grid, s_bc, None)
        self._check(self._dll.phihip_divergence_centered_backward(self.handle, byref(grid), bc, grad_out, grad_field, stream or None))

    def curl_2d(self, grid, staggered, vx, vy, s_bc, s_val, out, stream=0):
        """ staggered: vx / vy hold all faces; centred: vx is the (batch, 2, nx, ny) field and vy = 0 """
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_curl_2d(self.handle, byref(grid), int(bool(staggered)), vx, vy or None, bc, val, out, stream or None))

    def curl_2d_backward(self, grid, staggered, s_bc, grad_out, grad_vx, grad_vy, stream=0):
        bc, _ = _scalar_bc(grid, s_bc, None)
        self._check(self._dll.phihip_curl_2d_backward(self.handle, byref(grid), int(bool(staggered)), bc, grad_out, grad_vx, grad_vy or None,
            stream or None))

    # --- the finite-difference advection term (csrc/momentum.hpp); the *_backward entries accumulate, a gradient that is None is skipped ---
    def advect_differential(self, grid, u, u_batch, velocity, velocity_batch, out, stream=0):
        self._check(self._dll.phihip_advect_differential(self.handle, byref(grid), _ref3(u), int(u_batch), _ref3(velocity), int(velocity_batch),
            _ref3(out), stream or None))

    def advect_differential_backward(self, grid, u, velocity, grad_out, grad_u, grad_velocity, stream=0):
        self._check(self._dll.phihip_advect_differential_backward(self.handle, byref(grid), _ref3(u), _ref3(velocity), _ref3(grad_out),
            _ref3(grad_u), _ref3(grad_velocity), stream or None))

    def advect_differential_centered(self, grid, u, u_batch, s_bc, s_val, velocity, velocity_batch, out, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_advect_differential_centered(self.handle, byref(grid), u, int(u_batch), bc, val, velocity, int(velocity_batch),
            out, stream or None))

    def advect_differential_centered_backward(self, grid, u, s_bc, s_val, velocity, grad_out, grad_u, grad_velocity, stream=0):
        bc, val = _scalar_bc(grid, s_bc, s_val)
        self._check(self._dll.phihip_advect_differential_centered_backward(self.handle, byref(grid), u, bc, val, velocity, grad_out, grad_u or None,
            grad_velocity or None, stream or None))

    def diffuse_implicit_centered_coef(self, grid, s, s_bc, s_val, coef, c_batch, c_bc, c_val, kdt, out, solve: Solve, stream=0, want_info=True):
        """ diffuse.implicit with a varying / per-axis diffusivity; returns [batch] SolveInfo (None with want_info=False: no host read-back) """
        bc, val = _scalar_bc(grid, s_bc, s_val)
        cbc, cval = _scalar_bc(grid, c_bc if coef else s_bc, c_val if coef else s_val)
        info = (SolveInfo * grid.batch)() if want_info else None
        self._check(self._dll.phihip_diffuse_implicit_centered_coef(self.handle, byref(grid), s, bc, val, coef or None, int(c_batch), cbc, cval,
            _vec3(kdt), out, byref(solve), info, stream or None))
        return list(info) if want_info else None

    def profile_enable(self, enable: bool):
        self._check(self._dll.phihip_profile_enable(self.handle, int(bool(enable))))

    def profile_read(self, reset=True):
        launches = (c_int32 * K_COUNT)()
        ms = (c_double * K_COUNT)()
        self._check(self._dll.phihip_profile_read(self.handle, byref(launches), byref(ms), int(bool(reset))))
        return {K_NAMES[k]: (launches[k], ms[k]) for k in range(K_COUNT)}

    def set_tuning(self, rows_per_thread=0, threads_per_row=0, chunk_planes=0):
        self._check(self._dll.phihip_set_tuning(self.handle, int(rows_per_thread), int(threads_per_row), int(chunk_planes)))

    def set_tuning_kernel(self, family, rows_per_thread=0, threads_per_row=0, chunk_planes=0):
        """ family: 0 = apply / residual, 1 = MATVEC, 2 = UPDATE """
        self._check(self._dll.phihip_set_tuning_kernel(self.handle, int(family), int(rows_per_thread), int(threads_per_row), int(chunk_planes)))

    def set_small_grid_solver(self, enable):
        """ False / True, or an int > 1 = explicit cell limit of the single-kernel solver """
        self._check(self._dll.phihip_set_small_grid_solver(self.handle, int(enable)))

    def set_deferred_x_update(self, enable: bool):
        if callable(self._dll.phihip_set_deferred_x_update):      # (a no-op on the stand-in of a strict=False library that lacks the symbol)
            self._check(self._dll.phihip_set_deferred_x_update(self.handle, int(bool(enable))))

    def workspace_placement(self, candidates: int = -1) -> dict:
        """ Candidate allocations of the CG workspace the first solve on a freshly grown workspace chooses from (include/phihip.h phihip_workspace_placement):
        candidates 2 ... 16, 0 / 1 = keep the first allocation, -1 = unchanged. Returns the record of the most recent choice. """
        n = c_int32(0)
        us = (c_double * 2)(0.0, 0.0)
        self._check(self._dll.phihip_workspace_placement(self.handle, int(candidates), byref(n), us))
        return {"candidates": int(n.value), "us_first": float(us[0]), "us_kept": float(us[1])}

    def query_advect_chunk(self) -> int:
        """ planes per workgroup of the most recent tiled self-advection (0: none yet / 2-D) """
        out = c_int32(0)
        self._check(self._dll.phihip_query_advect_chunk(self.handle, byref(out)))
        return int(out.value)

    def set_advect_dma(self, enable: int = -1) -> bool:
        """ LDS-DMA fill of the tiled self-advection on regular grids (include/phihip.h): enable 1 / 0, -1 = unchanged. Returns whether the most
        recent tiled self-advection of this context took the LDS-DMA kernel. """
        out = c_int32(0)
        self._check(self._dll.phihip_set_advect_dma(self.handle, int(enable), byref(out)))
        return bool(out.value)

    def set_advect_windows_2d(self, enable: bool):
        """ LDS-windowed MacCormack / centred advection passes on 2-D grids as well (default: 3-D only; the gather kernels are faster in 2-D) """
        self._check(self._dll.phihip_set_advect_windows_2d(self.handle, int(bool(enable))))

    def set_advect_halo(self, halo: int):
        """ -1 (default): adaptive reach of the LDS-staged advection kernels; 0: gather kernels; 1 / 2: fixed reach in cells (include/phihip.h) """
        self._check(self._dll.phihip_set_advect_halo(self.handle, int(halo)))

    def allreduce_residual(self, comm, values_device, count, op=2, stream=0):
        """ in-place RCCL all-reduce of `count` device doubles over the caller's ncclComm_t (op 0 = sum, 2 = max); asynchronous """
        self._check(self._dll.phihip_allreduce_residual(self.handle, comm, values_device, int(count), int(op), stream or None))

    def set_single_reduction_cg(self, mode: int, max_cells: int = 0):
        """ 0: two launches per CG iteration always; 1: one fused launch per iteration for latency-bound solves (cells x batch <= max_cells,
        0 = built-in threshold); 2: always the fused form """
        self._check(self._dll.phihip_set_single_reduction_cg(self.handle, int(mode), int(max_cells)))

    def set_resident_cg(self, mode: int, max_cells: int = 0):
        """ resident solver for 2-D fp32 grids (the whole 'CG' solve in ONE launch, cg_resident.hip): 0 never, 1 when cells x batch <= max_cells
        (0 = keep the limit), 2 whenever applicable """
        self._check(self._dll.phihip_set_resident_cg(self.handle, int(mode), int(max_cells)))

    def set_autotune(self, enable: bool):
        """ first-call timing of the CG launch-plan candidates (default on; off = the analytic plan, reproducible launch geometry) """
        self._check(self._dll.phihip_set_autotune(self.handle, int(bool(enable))))

    def set_advect_chunk(self, planes: int):
        self._check(self._dll.phihip_set_advect_chunk(self.handle, int(planes)))

    def advect_fallback_stats(self, stream=0):
        """ (workgroups redone by the gather path, workgroups launched) of the most recent tiled self-advection; synchronises """
        out = (c_int32 * 2)()
        self._check(self._dll.phihip_advect_fallback_stats(self.handle, byref(out), stream or None))
        return out[0], out[1]

    def query_plan(self, grid, has_flags=False, family=1) -> dict:
        out = (c_int32 * 6)()
        self._check(self._dll.phihip_query_plan(self.handle, byref(grid), int(bool(has_flags)), int(family), byref(out)))
        return dict(rows=out[0], tpr=out[1], chunk=out[2], nblk=out[3], occupancy=out[4], vec=out[5])

    def workspace_bytes(self) -> int:
        out = c_size_t()
        self._check(self._dll.phihip_workspace_bytes(self.handle, byref(out)))
        return out.value


DEFAULT_LIBRARY_PATH = os.path.join(_HERE, "lib", "libphihip.so")
_default_library: Optional[Library] = None


def load_default_library() -> Library:
    """ loads phiflow_amd/lib/libphihip.so (built by ``__graft_entry__.build()``); raises `PhiHipLibraryError` if absent. """
    global _default_library
    if _default_library is None:
        override = os.environ.get("PHIHIP_LIBRARY")          # A/B measurements of another BUILD of libphihip (tools/): never a fallback
        if override:
            _default_library = Library(override, strict=False)
            return _default_library
        if not os.path.exists(DEFAULT_LIBRARY_PATH):
            raise PhiHipLibraryError(f"{DEFAULT_LIBRARY_PATH} does not exist. Build the HIP extension first "
                                     f"(`make -C phiflow_amd/csrc` or `__graft_entry__.build()`); phiflow_amd has no CPU fallback.")
        _default_library = Library(DEFAULT_LIBRARY_PATH)
    return _default_library

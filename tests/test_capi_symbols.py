"""
`-m "not gpu"`: the real gfx950 library loads in a GPU-less container and exports every symbol include/phihip.h declares; no
compute call is made (there is no CPU fallback: creating a context must fail loudly).
"""
import os
import re

import pytest

from phiflow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "phihip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(phihip_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(_capi.EXPORTED_SYMBOLS)


@pytest.mark.skipif(not os.path.exists(_capi.DEFAULT_LIBRARY_PATH), reason="libphihip.so not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    import ctypes
    dll = ctypes.CDLL(_capi.DEFAULT_LIBRARY_PATH)
    for name in _declared_symbols():
        assert hasattr(dll, name), f"{name} declared in include/phihip.h but not exported"
    lib = _capi.Library(_capi.DEFAULT_LIBRARY_PATH)
    assert lib.version() == 102


@pytest.mark.skipif(not os.path.exists(_capi.DEFAULT_LIBRARY_PATH), reason="libphihip.so not built")
def test_library_was_built_from_the_sources_in_this_tree():
    """ the .so is not in git and travels to the GPU box as a file: its embedded source hash must match the sources next to it """
    import subprocess
    lib = _capi.Library(_capi.DEFAULT_LIBRARY_PATH)
    if not lib.built_from_tree() and os.path.exists("/opt/rocm/bin/hipcc"):      # sources edited since the last build: rebuild, like build()
        # (flock: a second make on the same build directory -- another test session, a developer's shell -- must not interleave object files)
        csrc = os.path.join(ROOT, "phiflow_amd", "csrc")
        subprocess.run(["flock", os.path.join(csrc, ".build.lock"), "make", "-C", csrc, f"-j{min(16, os.cpu_count() or 4)}"], check=True, stdout=subprocess.DEVNULL)
        lib = _capi.Library(_capi.DEFAULT_LIBRARY_PATH)
    bid = lib.build_id()
    assert re.fullmatch(r"[0-9a-f]{12}(\+dirty)? src:[0-9a-f]{16}|nogit src:[0-9a-f]{16}", bid), bid
    assert lib.built_from_tree(), f"stale libphihip.so: built from {bid}, tree has src:{_capi.source_hash()} -- run __graft_entry__.build()"


@pytest.mark.skipif(not os.path.exists(_capi.DEFAULT_LIBRARY_PATH), reason="libphihip.so not built")
def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _capi.Library(_capi.DEFAULT_LIBRARY_PATH)
    with pytest.raises(_capi.PhiHipError) as e:
        _capi.Context(lib, 0)
    assert e.value.status == -4 and "no CPU fallback" in str(e.value)
    from phiflow_amd.backend import HipBackend
    with pytest.raises(RuntimeError):
        HipBackend()


def test_struct_layouts_match_the_header():
    import ctypes
    assert ctypes.sizeof(_capi.Grid) == 4 * 3 + 4 * 3 + 8 * 3 + 8 * 3 + 4 * 6 + 8 * 18
    assert ctypes.sizeof(_capi.Solve) == 32
    assert ctypes.sizeof(_capi.SolveInfo) == 32
    assert ctypes.sizeof(_capi.ObstacleStruct) == 4 * 4 + 8 * (3 + 3 + 3 + 3 + 9)      # kind, group, embed_mask, reserved + 21 doubles
    assert ctypes.sizeof(_capi.SdfGridStruct) == 8 + 4 * 6 + 8 * (3 + 3 + 3 + 1)


# ---- the binding is derived from include/phihip.h: pinned signatures, struct fields, constants, wrapper marshalling ----

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phihip.h")).read(), flags=re.S)


def _declared_parameters():
    """ {entry point: [parameter declaration, ...]} by a parse of this module's own """
    protos = re.findall(r"\b(phihip_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", _header_text())
    return {name: [" ".join(p.split()) for p in params.split(",") if p.strip() != "void"] for name, params in protos}


def test_pinned_signatures():
    """ the ctypes lists the binding had while it was written by hand, for entry points that together use every parameter spelling of the header """
    from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_longlong, c_size_t, c_void_p
    C = _capi
    p3, bc, val, grid, solve, info = POINTER(c_void_p * 3), POINTER((c_int32 * 2) * 3), POINTER((c_double * 2) * 3), POINTER(C.Grid), POINTER(C.Solve), POINTER(C.SolveInfo)
    pinned = {
        "phihip_ctx_create": [c_int, POINTER(c_void_p)],
        "phihip_workspace_bytes": [c_void_p, POINTER(c_size_t)],
        "phihip_component_shape": [grid, c_int, POINTER(c_int32 * 3)],
        "phihip_grid_sample": [c_void_p, grid, c_void_p, c_int, p3, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
        "phihip_make_incompressible": [c_void_p, grid, p3, p3, c_void_p, c_int, c_int, c_void_p, c_void_p, solve, info, c_void_p],
        "phihip_centered_to_staggered": [c_void_p, grid, c_void_p, bc, val, POINTER(c_double * 3), c_int, p3, c_void_p],
        "phihip_diffuse_implicit_centered_coef": [c_void_p, grid, c_void_p, bc, val, c_void_p, c_int, bc, val, POINTER(c_double * 3), c_void_p, solve, info, c_void_p],
        "phihip_profile_read": [c_void_p, POINTER(c_int32 * 9), POINTER(c_double * 9), c_int],
        # (`double last_us[2]` was POINTER(c_double) by hand; as an array parameter like every other it is POINTER(c_double * 2), which the wrapper's array satisfies)
        "phihip_workspace_placement": [c_void_p, c_int, POINTER(c_int32), POINTER(c_double * 2)],
        "phihip_set_resident_cg": [c_void_p, c_int, c_longlong],
        "phihip_query_plan": [c_void_p, grid, c_int, c_int, POINTER(c_int32 * 6)],
        "phihip_query_multigrid": [c_void_p, POINTER(c_int32 * 2)],
        "phihip_sdf_bind": [c_void_p, POINTER(C.SdfGridStruct), POINTER(c_int32)],
        "phihip_sdf_from_analytic": [c_void_p, POINTER(C.SdfGridStruct), POINTER(C.ObstacleStruct), c_int, c_void_p, c_void_p],
        "phihip_slab_state": [c_void_p, grid, c_int, c_void_p, solve, info, c_int, c_void_p],
        "phihip_solve_residuals": [c_void_p, c_int, c_void_p, c_void_p],
        "phihip_set_multigrid": [c_void_p, c_int, c_int, c_int, c_double],      # (the scalars `double` and `int32_t`, which none of the above has)
        "phihip_sdf_release": [c_void_p, c_int32],
    }
    for name, argtypes in pinned.items():
        assert C.SIGNATURES[name][1] == argtypes, name
        assert C.SIGNATURES[name][0] is c_int, name
    assert C.SIGNATURES["phihip_build_id"] == (c_char_p, []) and C.SIGNATURES["phihip_version"] == (c_int, [])
    # the pinned set covers the header: no other entry point uses a ctypes object that is not pinned above, and the 27 spellings are all there
    assert {t for _, argtypes in C.SIGNATURES.values() for t in argtypes} == {t for argtypes in pinned.values() for t in argtypes}
    spelling = lambda decl: re.sub(r"\s*\w+((?:\[\w+\])*)$", r"\1", decl.replace("const ", "").replace(" const", ""))   # noqa: E731
    declared = _declared_parameters()
    assert {spelling(d) for name in pinned for d in declared[name]} == {spelling(d) for params in declared.values() for d in params}
    assert len({spelling(d) for params in declared.values() for d in params}) == 27


def test_signatures_reach_the_loaded_library():
    """ Library sets what the header declares on every function of the table, over a stand-in of ctypes.CDLL (no library needed) """
    import ctypes

    class Function:
        pass

    class Dll:
        def __init__(self, path):
            for name in _declared_symbols():
                if name != "phihip_set_deferred_x_update":      # (a library that lacks a symbol: strict=False only)
                    setattr(self, name, Function())
    import torch  # noqa: F401  (Library imports it, and importing it loads libraries: before CDLL is replaced)
    real, ctypes.CDLL = ctypes.CDLL, Dll
    try:
        with pytest.raises(_capi.PhiHipLibraryError, match="phihip_set_deferred_x_update"):
            _capi.Library("libphihip.so")
        lib = _capi.Library("libphihip.so", strict=False)
    finally:
        ctypes.CDLL = real
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        if name != "phihip_set_deferred_x_update":
            assert getattr(lib.dll, name).restype is restype and getattr(lib.dll, name).argtypes == argtypes, name
    assert not callable(lib.dll.phihip_set_deferred_x_update)
    lib.dll.phihip_ctx_create = lambda device, out: 0
    _capi.Context(lib, 0).set_deferred_x_update(True)           # a no-op, not an error


def test_struct_fields_match_the_header():
    """ name, element type, array shape, order and offset (natural alignment of the header's types) of every field of the five structures """
    import ctypes
    elements = {"int32_t": (ctypes.c_int32, 4), "double": (ctypes.c_double, 8), "const void*": (ctypes.c_void_p, 8)}
    structs = {"phihip_grid": _capi.Grid, "phihip_solve": _capi.Solve, "phihip_solve_info": _capi.SolveInfo, "phihip_obstacle": _capi.ObstacleStruct,
               "phihip_sdf_grid": _capi.SdfGridStruct}
    bodies = dict(re.findall(r"typedef struct (\w+) \{(.*?)\}", _header_text(), flags=re.S))
    assert set(bodies) == set(structs)
    for cname, cls in structs.items():
        fields = re.findall(r"([\w ]+?\*?)\s*\b(\w+)((?:\[\d+\])*)\s*;", bodies[cname])
        assert [name for _, name, _ in fields] == [name for name, _ in cls._fields_], cname
        offset = 0
        for (elem, name, shape), (_, ctype) in zip(fields, cls._fields_):
            expected, size = elements[elem.strip()]
            for n in reversed([int(n) for n in re.findall(r"\d+", shape)]):
                expected = expected * n
            assert ctype is expected, (cname, name)
            offset = -(-offset // size) * size
            assert getattr(cls, name).offset == offset, (cname, name)
            offset += ctypes.sizeof(expected)
        assert ctypes.sizeof(cls) == -(-offset // 8) * 8, cname


def test_constants_are_the_headers():
    C = _capi
    assert C.K_NAMES == ("advect", "divergence", "cg_residual", "cg_matvec_dot", "cg_update", "cg_scalar", "grad_subtract", "other", "cg_update_r")
    assert C.K_COUNT == 9
    assert C.STATUS_NAMES == {0: "PHIHIP_OK", -1: "PHIHIP_ERR_BAD_ARG", -2: "PHIHIP_ERR_HIP", -3: "PHIHIP_ERR_UNSUPPORTED", -4: "PHIHIP_ERR_NO_DEVICE",
                              -5: "PHIHIP_ERR_ALLOC"}
    assert (C.PHIHIP_F32, C.PHIHIP_F64) == (0, 1) and (C.BC_PERIODIC, C.BC_CLOSED, C.BC_OPEN) == (0, 1, 2)
    assert (C.OBSTACLE_BOX, C.OBSTACLE_SPHERE, C.OBSTACLE_SDF, C.OBSTACLE_CYLINDER) == (0, 1, 2, 3)
    assert C.SDF_SLOTS == 64 and (C.DIV_BALANCE, C.DIV_FINITE_GUARD) == (1, 4) and C.VERSION == 102
    from phiflow_amd.solve import Solve
    assert Solve.METHODS == {"auto": C.CONSTANTS["PHIHIP_METHOD_CG"], "CG": C.CONSTANTS["PHIHIP_METHOD_CG"], "CG-adaptive": C.CONSTANTS["PHIHIP_METHOD_CG_ADAPTIVE"]}
    assert Solve.METHOD_CG_MULTIGRID == C.CONSTANTS["PHIHIP_METHOD_CG_MULTIGRID"]


def test_unknown_spelling_is_an_error():
    _capi.load_header("#define PHIHIP_N 4\nint phihip_fine(phihip_ctx* ctx, const int32_t out[PHIHIP_N], void* stream);")
    for decl, spelling in (("float weight", "float"), ("const int16_t* flags", "int16_t*"), ("double m[3][3]", "double[3][3]"), ("int32_t out[PHIHIP_M]", "int32_t[PHIHIP_M]")):
        with pytest.raises(_capi.PhiHipLibraryError) as e:
            _capi.load_header(f"int phihip_fine(phihip_ctx* ctx);\nint phihip_odd(phihip_ctx* ctx, {decl}, void* stream);")
        assert "phihip_odd" in str(e.value) and f"'{spelling}'" in str(e.value) and decl in str(e.value)
    with pytest.raises(_capi.PhiHipLibraryError, match="phihip_odd.*'float'"):
        _capi.load_header("float phihip_odd(phihip_ctx* ctx);")


# ---- wrapper marshalling over a stand-in library: what reaches the C side ----

class _Recorder:
    """ stands in for the loaded library: every phihip_* attribute is a callable that records its arguments and returns 0 """

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("phihip_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


A, B, C3, D, E, F = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000      # "device pointers"
S_BC, S_VAL = ((0, 0), (2, 1)), ((0.0, 0.0), (0.5, -1.5))
C_BC, C_VAL = ((2, 2), (1, 1)), ((0.0, 0.0), (3.0, 4.0))


def _stand_in():
    lib = _capi.Library.__new__(_capi.Library)
    lib.dll = _Recorder()
    ctx = _capi.Context(lib, 0)
    grid = _capi.make_grid(2, _capi.PHIHIP_F32, 2, (8, 6), (0, 0), (1, 1), ((0, 0), (1, 2)))      # rank 2: third components unused; batch 2
    return ctx, lib.dll.calls, grid, _capi.Solve(1e-5, 0.0, 100, 50, 10, 0)


def _nested(ref):
    """ the array behind a byref argument as nested lists """
    def listed(a):
        return [listed(x) for x in a] if hasattr(a, "_length_") else a
    return listed(ref._obj)


def _drives(grid, solve):
    """ one call of every public wrapper: {wrapper: (args, kwargs)}; every OPTIONAL device pointer is 0 or None, every required one non-zero """
    obstacles, desc = _capi.make_obstacles([dict(kind=_capi.OBSTACLE_SPHERE, center=(0.5, 0.5), half_size=(0.1,))]), \
        _capi.make_sdf_grid(A, _capi.PHIHIP_F32, (4, 4), (0, 0), (1, 1), (0.5, 0.5), 0.7, True)
    V, W = [A, B], [C3, D]
    return {
        "component_shape": ((grid, 1), {}),
        "advect_staggered": ((grid, V, V, W, 0.25), {}),
        "advect_centered": ((grid, E, S_BC, S_VAL, V, F, 0.5), {}),
        "advect_centered_vector": ((grid, A, 1, 2, S_BC, S_VAL, B, 2, C3, 0.5), {}),
        "staggered_to_centered": ((grid, V, E), {}),
        "centered_vector_to_staggered": ((grid, E, 1, S_BC, S_VAL, W), {}),
        "grid_sample": ((grid, E, 1, V, 2 ** 33, 0), {}),
        "grid_sample_backward": ((grid, E, 1, V, 5, F, 0, None), {}),
        "mac_cormack_staggered": ((grid, V, V, W, 0.25), {}),
        "mac_cormack_centered": ((grid, E, S_BC, S_VAL, V, F, 0.5, 0.75), {}),
        "centered_to_staggered": ((grid, E, S_BC, S_VAL, (0.0, 0.1), True, W), {}),
        "advect_staggered_backward": ((grid, V, V, W, 0.25, None, None), {}),
        "advect_centered_backward": ((grid, E, S_BC, S_VAL, V, F, 0.5, 0, None), {}),
        "mac_cormack_staggered_backward": ((grid, V, V, W, 0.25, 1.0, W, None), {}),
        "mac_cormack_centered_backward": ((grid, E, S_BC, S_VAL, V, F, 0.5, 1.0, A, None), {}),
        "diffuse_explicit_backward": ((grid, V, W, 0.1), {}),
        "diffuse_explicit_centered": ((grid, E, S_BC, S_VAL, F, 0.1), {}),
        "centered_to_staggered_backward": ((grid, S_BC, (0.0, 0.1), V, E), {}),
        "make_incompressible_backward": ((grid, 0, 1, 5, V, 0, solve), {}),
        "slab_residual": ((grid, (1, 0), 0, A, (B, 0), C3, D, E), {}),
        "slab_matvec": ((grid, (1, 0), 0, True, A, B, (C3, 0), D, (0, E), F, A, solve), {}),
        "slab_update": ((grid, (0, 1), 0, A, B, (0, C3), D, 0, 0, solve), {}),
        "slab_state": ((grid, True, A, solve), {}),
        "obstacle_accessible": ((grid, obstacles, 1, A), {}),
        "apply_obstacles": ((grid, obstacles, 1, V), {}),
        "sdf_bind": ((desc,), {}),
        "sdf_release": ((3,), {}),
        "sdf_from_analytic": ((desc, obstacles, 1, B), {}),
        "build_cellflags": ((grid, 0, 0, 1, A), {}),
        "divergence": ((grid, V, 0, 1, 1, E), {}),
        "laplace_apply": ((grid, 0, 1, E, F), {}),
        "cg_solve": ((grid, 0, 1, E, F, solve), {}),
        "precondition_apply": ((grid, 0, 1, E, F), {}),
        "set_multigrid": ((3, 4, 20, 0.7), {}),
        "query_multigrid": ((), {}),
        "cg_solve_shifted": ((grid, 1.0, -0.5, E, F, solve), {}),
        "solve_residuals": ((2, A), {}),
        "solve_relative_residual": ((2, A), {}),
        "grad_subtract": ((grid, 0, 1, E, V), {}),
        "make_incompressible": ((grid, V, None, 0, 1, 1, E, 0, solve), {}),
        "diffuse_explicit": ((grid, V, W, 0.1), {}),
        "diffuse_implicit": ((grid, V, W, 0.1, solve), {}),
        "diffuse_implicit_centered": ((grid, E, S_BC, S_VAL, F, 0.1, solve), {}),
        "diffuse_explicit_centered_coef": ((grid, E, S_BC, S_VAL, 0, 1, C_BC, C_VAL, (0.1, 0.2), F), {}),
        "field_laplace": ((grid, V, W, 1.0), {}),
        "field_laplace_centered": ((grid, E, S_BC, S_VAL, (1.0, 2.0), F), {}),
        "gradient_centered": ((grid, E, S_BC, S_VAL, F), {}),
        "gradient_centered_backward": ((grid, S_BC, E, F), {}),
        "divergence_centered": ((grid, E, S_BC, S_VAL, F), {}),
        "divergence_centered_backward": ((grid, S_BC, E, F), {}),
        "curl_2d": ((grid, False, E, 0, S_BC, S_VAL, F), {}),
        "curl_2d_backward": ((grid, False, S_BC, E, F, 0), {}),
        "advect_differential": ((grid, V, 1, V, 2, W), {}),
        "advect_differential_backward": ((grid, V, V, W, None, None), {}),
        "advect_differential_centered": ((grid, E, 1, S_BC, S_VAL, F, 2, A), {}),
        "advect_differential_centered_backward": ((grid, E, S_BC, S_VAL, F, A, 0, 0), {}),
        "diffuse_implicit_centered_coef": ((grid, E, S_BC, S_VAL, 0, 1, C_BC, C_VAL, (0.1, 0.2), F, solve), {}),
        "profile_enable": ((True,), {}),
        "profile_read": ((), {}),
        "set_tuning": ((1, 64, 4), {}),
        "set_tuning_kernel": ((2, 1, 64, 4), {}),
        "set_small_grid_solver": ((True,), {}),
        "set_deferred_x_update": ((False,), {}),
        "workspace_placement": ((), {}),
        "query_advect_chunk": ((), {}),
        "set_advect_dma": ((), {}),
        "set_advect_windows_2d": ((True,), {}),
        "set_advect_halo": ((2,), {}),
        "allreduce_residual": ((A, B, 4), {}),
        "set_single_reduction_cg": ((1, 2 ** 40), {}),
        "set_resident_cg": ((1,), {}),
        "set_autotune": ((False,), {}),
        "set_advect_chunk": ((8,), {}),
        "advect_fallback_stats": ((), {}),
        "query_plan": ((grid,), {}),
        "workspace_bytes": ((), {}),
    }


def test_every_wrapper_passes_the_declared_arguments():
    """ every public wrapper of Context, driven once: as many arguments as the prototype declares, the context first, and no integer 0 where a pointer is
    declared (an optional device pointer given as 0 must arrive as NULL, i.e. None: ctypes would pass the int 0 to a c_void_p all the same, but a
    wrapper that forgets `or None` also forgets it where the parameter is a typed pointer) """
    ctx, calls, grid, solve = _stand_in()
    drives = _drives(grid, solve)
    public = sorted(n for n, f in vars(_capi.Context).items() if callable(f) and not n.startswith("_") and n != "close")
    assert public == sorted(drives)
    declared = _declared_parameters()
    for name, (args, kwargs) in drives.items():
        del calls[:]
        getattr(ctx, name)(*args, **kwargs)
        assert [c[0] for c in calls] == ["phihip_" + name], name
        passed, params = calls[0][1], declared["phihip_" + name]
        assert len(passed) == len(params), (name, len(passed), params)
        if params[0] == "phihip_ctx* ctx":
            assert passed[0] is ctx.handle, name
        for value, decl in zip(passed, params):
            if "*" in decl or "[" in decl:
                assert not isinstance(value, (int, float)) or value != 0, (name, decl)
            else:
                assert type(value) is (float if decl.startswith("double") else int), (name, decl, value)


def test_wrapper_marshalling():
    """ what reaches the C side, for one wrapper of each family """
    ctx, calls, grid, solve = _stand_in()
    h = ctx.handle

    def last():
        return calls[-1][1]
    # staggered, three pointers: trailing component of a rank-2 field NULL; stream 0 -> NULL, a stream passes
    ctx.advect_staggered(grid, [A, B], [A, B], [C3, D], 0.25)
    a = last()
    assert a[0] is h and a[1]._obj is grid and [_nested(x) for x in a[2:5]] == [[A, B, None], [A, B, None], [C3, D, None]] and a[5:] == (0.25, None)
    ctx.advect_staggered(grid, [A, B, 0], [A, B, 0], [C3, D, 0], 1, stream=77)
    assert _nested(last()[2]) == [A, B, None] and last()[5:] == (1.0, 77) and type(last()[5]) is float
    # centred with s_bc / s_val: the axes of the grid's rank filled, the rest zero
    ctx.advect_centered(grid, E, S_BC, S_VAL, [A, B], F, 0.5)
    a = last()
    assert a[2] == E and _nested(a[3]) == [[0, 0], [2, 1], [0, 0]] and _nested(a[4]) == [[0.0, 0.0], [0.5, -1.5], [0.0, 0.0]]
    assert _nested(a[5]) == [A, B, None] and a[6:] == (F, 0.5, None)
    ctx.gradient_centered_backward(grid, S_BC, E, F)             # s_val = None: no values are passed at all
    assert _nested(last()[2]) == [[0, 0], [2, 1], [0, 0]] and last()[3:] == (E, F, None) and len(last()) == 6
    ctx.centered_to_staggered(grid, E, S_BC, S_VAL, (0.0, 0.1), True, [C3, D])
    assert _nested(last()[5]) == [0.0, 0.1, 0.0] and last()[6] == 1 and _nested(last()[7]) == [C3, D, None]
    # coefficient diffusion: coef = 0 is NULL and its extrapolation falls back to the field's
    ctx.diffuse_explicit_centered_coef(grid, E, S_BC, S_VAL, 0, 1, C_BC, C_VAL, (0.1, 0.2), F, adjoint=True)
    a = last()
    assert a[5] is None and a[6] == 1 and _nested(a[7]) == _nested(a[3]) == [[0, 0], [2, 1], [0, 0]] and _nested(a[8]) == _nested(a[4])
    assert _nested(a[9]) == [0.1, 0.2, 0.0] and a[10:] == (F, 1, None)
    ctx.diffuse_explicit_centered_coef(grid, E, S_BC, S_VAL, A, 2, C_BC, C_VAL, (0.1, 0.2), F)
    a = last()
    assert a[5] == A and a[6] == 2 and _nested(a[7]) == [[2, 2], [1, 1], [0, 0]] and _nested(a[8]) == [[0.0, 0.0], [3.0, 4.0], [0.0, 0.0]] and a[11] == 0
    assert ctx.diffuse_implicit_centered_coef(grid, E, S_BC, S_VAL, 0, 1, C_BC, C_VAL, (0.1, 0.2), F, solve, want_info=False) is None
    a = last()
    assert a[5] is None and _nested(a[7]) == _nested(a[3]) and a[11]._obj is solve and a[12:] == (None, None)
    # a solve without and with info
    assert ctx.make_incompressible(grid, [A, B], None, 0, 1, 1, E, 0, solve, want_info=False) is None
    a = last()
    assert _nested(a[2]) == [A, B, None] and a[3] is None and a[4] is None and a[5:9] == (1, 1, E, None) and a[9]._obj is solve and a[10:] == (None, None)
    info = ctx.make_incompressible(grid, [A, B], [C3, D], F, 2, 5, E, A, solve, stream=9)
    a = last()
    assert _nested(a[3]) == [C3, D, None] and a[4:9] == (F, 2, 5, E, A) and a[11] == 9
    assert isinstance(a[10], _capi.SolveInfo * 2) and isinstance(info, list) and len(info) == 2 and all(isinstance(i, _capi.SolveInfo) for i in info)
    assert len(ctx.cg_solve(grid, 0, 1, E, F, solve)) == 2 and last()[2] is None and ctx.cg_solve(grid, A, 1, E, F, solve, want_info=False) is None
    assert len(ctx.diffuse_implicit(grid, [A, B], [C3, D], 0.1, solve)) == 4 and isinstance(last()[6], _capi.SolveInfo * 4)      # rank x batch
    assert ctx.diffuse_implicit(grid, [A, B], [C3, D], 0.1, solve, want_info=False) is None and last()[6] is None
    assert len(ctx.slab_state(grid, True, A, solve, peek=True)) == 2 and last()[2:4] == (1, A) and last()[6:] == (1, None)
    # backward passes: a gradient that is None is NULL; the balance bits are masked
    ctx.advect_staggered_backward(grid, [A, B], [A, B], [C3, D], 0.25, None, [E, F])
    assert last()[6] is None and _nested(last()[7]) == [E, F, None]
    ctx.advect_differential_backward(grid, [A, B], [A, B], [C3, D], [E, F], None)
    assert _nested(last()[5]) == [E, F, None] and last()[6] is None
    ctx.grid_sample_backward(grid, E, 1, [A, B], 5, F, 0, None)
    assert last()[7:] == (None, None, None)
    ctx.make_incompressible_backward(grid, 0, 1, _capi.DIV_BALANCE | _capi.DIV_FINITE_GUARD, [A, B], 0, solve, want_info=False)
    a = last()
    assert a[2:5] == (None, 1, _capi.DIV_BALANCE) and _nested(a[5]) == [A, B, None] and a[6] is None and a[8:] == (None, None)
    # slab phases: a zero halo pointer is NULL
    ctx.slab_matvec(grid, (1, 0), 0, True, A, B, (C3, 0), D, (0, E), F, A, solve)
    a = last()
    assert a[2:16] == (1, 0, None, 1, A, B, C3, None, D, None, E, F, A, a[15]) and a[15]._obj is solve
    ctx.slab_residual(grid, (0, 1), A, B, (0, C3), D, E, F, keep_going=True)
    assert last()[2:] == (0, 1, A, B, None, C3, D, E, F, 1, None)
    ctx.slab_update(grid, (1, 1), 0, A, B, (C3, D), E, 0, 0, solve, x_only=True)
    assert last()[4:13] == (None, A, B, C3, D, E, None, None, 1)
    # set_* / query_* / the call without a context
    ctx.set_tuning(1, 64, 4)
    assert last() == (h, 1, 64, 4)
    ctx.set_resident_cg(True, 2 ** 40)
    assert last() == (h, 1, 2 ** 40)
    assert set(ctx.query_plan(grid, has_flags=True)) == {"rows", "tpr", "chunk", "nblk", "occupancy", "vec"} and last()[2:4] == (1, 1)
    assert ctx.workspace_placement() == {"candidates": 0, "us_first": 0.0, "us_kept": 0.0} and last()[1] == -1
    assert set(ctx.profile_read()) == set(_capi.K_NAMES) and last()[3] == 1
    assert ctx.component_shape(grid, 1) == (0, 0) and last()[0]._obj is grid and last()[1] == 1 and len(last()) == 3
    ctx.build_cellflags(grid, 0, B, 1, A)
    assert last()[2:] == (None, B, 1, A, None)

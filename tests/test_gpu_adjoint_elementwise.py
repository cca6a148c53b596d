"""
`-m gpu`: element-wise parity of the adjoint kernels on the MI355X, in fp32 and fp64 -- the cases of tests/test_adjoint_elementwise_emu.py through device
memory, and the sizes the emulation is too slow for: (48, 40, 136) and (40, 36, 384), a row of 264 cells, and one 256^3 fp32 periodic staggered case, the only
size where the adjoint launches reach their 65 536-block cap. Yardstick and comparison rule: tests/adjoint_cases.py. Every case prints its figures.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import adjoint_cases as A
import parity_cases as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
_id = A.case_id


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("case", A.TILE_CASES, ids=_id)
def test_every_entry_point_on_tile_edges(ctx, mem, case, dtype):
    res, bc, batch, dt, k0, slab_axis = case
    A.run_case(ctx, mem, res, bc, dtype, batch, dt, seed=1, k0=k0, slab_axis=slab_axis, flip=len(res) == 3 and res[0] % 2 == 1)


@DTYPES
@pytest.mark.parametrize("case", A.SMALL_CASES, ids=_id)
def test_every_entry_point_on_axes_of_one_to_three_cells(ctx, mem, case, dtype):
    res, bc, batch = case
    A.run_case(ctx, mem, res, bc, dtype, batch, 0.7, seed=2, flip=True)
    A.run_case(ctx, mem, res, bc, dtype, batch, 2.9, seed=5, k0=-1, entries=A.ENTRIES[:4])


@DTYPES
@pytest.mark.parametrize("case", A.LARGE_CASES, ids=_id)
def test_every_entry_point_on_large_grids(ctx, mem, case, dtype):
    res, bc, batch, dt, k0, slab_axis = case
    A.run_case(ctx, mem, res, bc, dtype, batch, dt, seed=4, k0=k0, slab_axis=slab_axis)


@DTYPES
@pytest.mark.parametrize("case", A.CHUNKED_DIFFUSE_CASES, ids=_id)
def test_diffuse_adjoints_march_several_planes(ctx, mem, case, dtype):
    """ a thin grid of many planes: every workgroup of the diffuse adjoints carries its a0 neighbours over a chunk of two planes """
    res, bc, batch = case
    A.run_case(ctx, mem, res, bc, dtype, batch, seed=3, entries=('diffuse',))


def test_extruded_256_cubed_fp32_reaches_the_block_cap(ctx, mem):
    """ 256^3 periodic staggered advection of an extruded 2-D flow: every plane of the field gradient and of the in-plane velocity gradients against the 2-D
    reference of that plane """
    del A.RECORDS[:]
    try:
        A.check_extruded_staggered(ctx, mem, 256, (256, 256), np.float32, dt=0.7, seed=6)
    finally:
        A.report()


@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-batch", "shared"])
@pytest.mark.parametrize("case", A.GRID_SAMPLE_CASES, ids=_id)
def test_grid_sample_backward(ctx, mem, case, shared, dtype):
    A.run_grid_sample(ctx, mem, case[0], case[1], dtype, shared)


@pytest.mark.parametrize("case", A.PROJECT_CASES, ids=_id)
def test_projection_adjoint_fp32(ctx, mem, case):
    A.run_project_backward(ctx, mem, *case, np.float32)


def test_projection_adjoint_dense_with_obstacle(ctx, mem):
    A.check_project_backward_dense(ctx, mem)
    A.report()


def test_per_component_launch_form_is_correct():
    """ PHIHIP_ADJOINT_ALL=0 against the reference, in a fresh child process """
    env = dict(os.environ, PHIHIP_ADJOINT_ALL="0")
    out = subprocess.run([sys.executable, os.path.join(HERE, "adjoint_elementwise_probe.py"), "gpu"], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "PHIHIP_ADJOINT_ALL = 0" in out.stdout and "probe ok" in out.stdout


def test_per_axis_factors_with_constant_walls_regression(ctx, mem):
    """ the device side of tests/test_adjoint_elementwise_emu.py::test_per_axis_factors_with_constant_walls_regression """
    import diffuse_coef_ref
    codes, vals = ((pc.CLO, pc.CLO), (pc.CLO, pc.OPN)), [(0.7, -0.5), (0.3, 0.0)]
    for dtype, bound in ((np.float64, pc.TOL64['stencil']), (np.float32, pc.TOL32['stencil'])):
        dom, grid = pc.make_case((6, 5), ((pc.OPN, pc.OPN),) * 2, dtype, 2)
        u = np.random.default_rng(0).standard_normal((2, 6, 5)).astype(dtype)
        du, out = mem.to_dev(u), mem.empty(u.shape, dtype)
        ctx.diffuse_explicit_centered_coef(grid, mem.ptr(du), codes, vals, 0, 1, codes, vals, [0.1, 0.2], mem.ptr(out))
        mem.sync()
        ref = diffuse_coef_ref.explicit(u.astype(np.float64), None, [0.1, 0.2], dom.dx, codes, vals)
        err = pc.rel_err(mem.to_host(out).astype(np.float64), ref)
        print(f"per-axis factors, constant walls, {np.dtype(dtype).name}: {err:.3e}")
        assert err <= bound, err

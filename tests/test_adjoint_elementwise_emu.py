"""
Element-wise parity of the adjoint kernels under the CPU emulation (tests/hipemu), in fp32 and fp64: every gradient array of every backward entry point
against torch.autograd through a float64 restatement of the oracle's forward functions (tests/adjoint_ref.py, tests/adjoint_cases.py -- the comparison
rule, the constructed fp32 inputs and the treatment of undecided limiter samples are described there). Each test asserts, inside the checks it calls, the pin
of the restatement to the oracle's forward (<= 1e-12), the margin of every lookup coordinate and the <= 1 % cap of zeroed samples. tests/test_gpu_adjoint_elementwise.py
repeats the cases on the device. Every case prints its figures.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import adjoint_cases as A
import parity_cases as pc

MEM = pc.NumpyMem()
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


_id = A.case_id


@DTYPES
@pytest.mark.parametrize("case", A.TILE_CASES, ids=_id)
def test_every_entry_point_on_tile_edges(emu_ctx, case, dtype):
    """ extents one below, at and one above a multiple of pass B's tile, tiles on the `inside` path next to ragged ones, components of unequal shapes, samples
    inside and outside their neighbourhood in one launch """
    res, bc, batch, dt, k0, slab_axis = case
    A.run_case(emu_ctx, MEM, res, bc, dtype, batch, dt, seed=1, k0=k0, slab_axis=slab_axis, flip=len(res) == 3 and res[0] % 2 == 1)


@DTYPES
@pytest.mark.parametrize("case", A.SMALL_CASES, ids=_id)
def test_every_entry_point_on_axes_of_one_to_three_cells(emu_ctx, case, dtype):
    """ the ends of the array in pass C and in the centred -> staggered adjoint: ghost slots and periodic images of the same few samples """
    res, bc, batch = case
    A.run_case(emu_ctx, MEM, res, bc, dtype, batch, 0.7, seed=2, flip=True)
    A.run_case(emu_ctx, MEM, res, bc, dtype, batch, 2.9, seed=5, k0=-1, entries=A.ENTRIES[:4])


@DTYPES
@pytest.mark.parametrize("case", A.CHUNKED_DIFFUSE_CASES, ids=_id)
def test_diffuse_adjoints_march_several_planes(emu_ctx, case, dtype):
    """ a thin grid of many planes: every workgroup of the diffuse adjoints carries its a0 neighbours over a chunk of two planes """
    res, bc, batch = case
    A.run_case(emu_ctx, MEM, res, bc, dtype, batch, seed=3, entries=('diffuse',))


@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-batch", "shared"])
@pytest.mark.parametrize("case", A.GRID_SAMPLE_CASES, ids=_id)
def test_grid_sample_backward(emu_ctx, case, shared, dtype):
    A.run_grid_sample(emu_ctx, MEM, case[0], case[1], dtype, shared)


@pytest.mark.parametrize("case", A.PROJECT_CASES, ids=_id)
def test_projection_adjoint_fp32(emu_ctx, case):
    """ make_incompressible_backward in fp32 against the float64 oracle difference, to the fp32 CG tolerance """
    A.run_project_backward(emu_ctx, MEM, *case, np.float32)


def test_projection_adjoint_dense_with_obstacle(emu_ctx):
    """ the full Jacobian of the oracle's projection (unit vectors), transposed onto the cotangent: element by element """
    A.check_project_backward_dense(emu_ctx, MEM)
    A.report()


def test_per_component_launch_form_is_correct(emu_library):
    """ PHIHIP_ADJOINT_ALL=0 (one launch per component) against the reference, in a child process: the library reads the variable once """
    env = dict(os.environ, PHIHIP_ADJOINT_ALL="0", PHIHIP_AUTOTUNE="0")
    out = subprocess.run([sys.executable, os.path.join(HERE, "adjoint_elementwise_probe.py"), "emu"], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "PHIHIP_ADJOINT_ALL = 0" in out.stdout and "probe ok" in out.stdout


def test_per_axis_factors_with_constant_walls_regression(emu_ctx):
    """ found by the element-wise adjoint checks: diffuse_explicit_centered_coef WITHOUT a coefficient array (per-axis factors) took the ghost value of the
    coefficient from the scalar's own wall constant instead of 1, in the forward pass and in the adjoint alike: the face at a constant wall c conducted with
    min(1, c). Forward against tests/diffuse_coef_ref.py, fp64 to 1e-13 and fp32 to TOL32['stencil'], walls 0.7 / -0.5 / 0.3. """
    import diffuse_coef_ref
    codes, vals = ((pc.CLO, pc.CLO), (pc.CLO, pc.OPN)), [(0.7, -0.5), (0.3, 0.0)]
    for dtype, bound in ((np.float64, pc.TOL64['stencil']), (np.float32, pc.TOL32['stencil'])):
        dom, grid = pc.make_case((6, 5), ((pc.OPN, pc.OPN),) * 2, dtype, 2)
        u = np.random.default_rng(0).standard_normal((2, 6, 5)).astype(dtype)
        du, out = MEM.to_dev(u), MEM.empty(u.shape, dtype)
        emu_ctx.diffuse_explicit_centered_coef(grid, MEM.ptr(du), codes, vals, 0, 1, codes, vals, [0.1, 0.2], MEM.ptr(out))
        ref = diffuse_coef_ref.explicit(u.astype(np.float64), None, [0.1, 0.2], dom.dx, codes, vals)
        err = pc.rel_err(MEM.to_host(out).astype(np.float64), ref)
        print(f"per-axis factors, constant walls, {np.dtype(dtype).name}: {err:.3e}")
        assert err <= bound, err

"""
`-m gpu`: finite, rotated and moving cylinders (Cylinder / cylinder) on the MI355X -- the tables of tests/test_cylinder_emu.py through device memory:
the cylinder branch of the obstacle kernels element by element (rule, scenes, grids: tests/cylinder_cases.py), the refusals of the C ABI, fluid.py against the
composed C calls, dimension orders, unions and batches, the mask cache, jit_compile, the backward pass, sample_sdf and the example. Every case prints its figures.
"""
import numpy as np
import pytest

import cylinder_cases as CC
import parity_cases as pc
import test_cylinder_emu as host

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("case", CC.GRIDS, ids=CC.case_id)
def test_cylinder_kernels(ctx, mem, case, dtype):
    worst = CC.run_cylinder_obstacles(ctx, mem, case[0], case[1], dtype, case[2], seed=5)
    print(f"cylinder worst error / bound {worst:.3g} ({CC.case_id(case)}, {np.dtype(dtype).name})")
    assert worst <= 1.0


def test_c_abi_refusals(ctx, mem):
    host.check_c_abi_refusals(ctx, mem)


@DTYPES
def test_fluid_calls_equal_the_composed_c_calls(gpu_backend, dtype):
    host.test_fluid_calls_equal_the_composed_c_calls(gpu_backend, dtype)


def test_dimension_order_of_the_geometry_does_not_matter(gpu_backend):
    host.test_dimension_order_of_the_geometry_does_not_matter(gpu_backend)


def test_union_member_and_batched_radii(gpu_backend):
    host.test_union_member_and_batched_radii(gpu_backend)


def test_mask_cache_tells_close_cylinders_apart(gpu_backend):
    host.test_mask_cache_tells_close_cylinders_apart(gpu_backend)


def test_static_cylinder_under_jit_compile_replays_the_eager_bits(gpu_backend):
    host.test_static_cylinder_under_jit_compile_replays_the_eager_bits(gpu_backend)


def test_gradient_through_the_projection_equals_the_one_with_explicit_flags(gpu_backend):
    host.test_gradient_through_the_projection_equals_the_one_with_explicit_flags(gpu_backend)


@DTYPES
def test_sample_sdf_of_a_cylinder(gpu_backend, dtype):
    host.test_sample_sdf_of_a_cylinder(gpu_backend, dtype)


def test_python_refusals(gpu_backend):
    host.test_python_refusals(gpu_backend)


def test_example_runs(gpu_backend):
    host.test_example_runs(gpu_backend)

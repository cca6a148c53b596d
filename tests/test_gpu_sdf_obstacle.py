"""
`-m gpu`: obstacles from a signed-distance grid (SDFGrid) on the MI355X -- the tables of tests/test_sdf_obstacle_emu.py through device memory: the
kernels of phiflow_amd/csrc/obstacle_sdf.hpp element by element (rule, scenes, grids: tests/sdf_obstacle_cases.py), the refusals of the C ABI, sample_sdf on the
device, the projection, batched grids, the mask cache, the backward pass and the example. Every case prints its figures.
"""
import numpy as np
import pytest

import parity_cases as pc
import sdf_obstacle_cases as SC
import test_sdf_obstacle_emu as host

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def ctx(gpu_backend):
    return gpu_backend.ctx


@pytest.fixture(scope="module")
def mem(gpu_backend):
    return pc.TorchMem(str(gpu_backend.device))


@DTYPES
@pytest.mark.parametrize("case", SC.GRIDS, ids=SC.case_id)
def test_sdf_obstacle_kernels(ctx, mem, case, dtype):
    worst = SC.run_sdf_obstacles(ctx, mem, case[0], case[1], dtype, case[2], seed=5)
    print(f"sdf-obstacle worst error / bound {worst:.3g} ({SC.case_id(case)}, {np.dtype(dtype).name})")
    assert worst <= 1.0


def test_c_abi_refusals(gpu_backend):
    host.check_c_abi_refusals(gpu_backend.ctx, pc.TorchMem(str(gpu_backend.device)))


@DTYPES
def test_sample_sdf_against_the_host_distance(gpu_backend, dtype):
    host.test_sample_sdf_against_the_host_distance(gpu_backend, dtype)


def test_device_tensor_is_used_in_place(gpu_backend):
    """ an `sdf` tensor that already lives on the device is the array the kernels read: no second copy, kept alive by the geometry """
    import torch
    from phiflow_amd.flow import Box, SDFGrid
    vals = host._blob((9, 8), (2.0, 2.0), (9.0, 8.0), np.float32)
    t = torch.from_numpy(vals).to(gpu_backend.device)
    g = SDFGrid(t, Box(x=(2.0, 9.0), y=(2.0, 8.0)))
    assert g.device_values(gpu_backend).data_ptr() == t.data_ptr() and g.shifted((1.0, 0.0)).device_values(gpu_backend).data_ptr() == t.data_ptr()
    assert np.array_equal(g.values, vals)


def test_resample_and_where_take_an_sdf_grid(gpu_backend):
    host.test_resample_and_where_take_an_sdf_grid(gpu_backend)


def test_python_refusals(gpu_backend):
    host.test_python_refusals(gpu_backend)


def test_mask_cache_misses_after_shifted(gpu_backend):
    host.test_mask_cache_misses_after_shifted(gpu_backend)


@pytest.mark.parametrize("res", [(24, 20), (12, 10, 16)], ids=["24x20", "12x10x16"])
def test_projection_around_an_sdf_obstacle(gpu_backend, res):
    host.test_projection_around_an_sdf_obstacle(gpu_backend, res)


def test_batched_sdf_grid_gives_per_entry_masks(gpu_backend):
    host.test_batched_sdf_grid_gives_per_entry_masks(gpu_backend)


def test_functional_gradient_through_a_step_with_an_sdf_obstacle(gpu_backend):
    host.test_functional_gradient_through_a_step_with_an_sdf_obstacle(gpu_backend)


def test_example_runs(gpu_backend):
    host.test_example_runs(gpu_backend)

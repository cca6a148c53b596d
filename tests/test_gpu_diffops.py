"""
Grid differential operators on the MI355X (csrc/diffops.hpp; laplace through the marching kernels and coef_kernel<CM_LAP>): the element-wise
forward and backward checks, the hand values and the jit_compile replay of tests/diffops_cases.py on the device.
"""
import numpy as np
import pytest

from phiflow_amd.flow import PERIODIC, CenteredGrid, jit_compile, precision

import diffops_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_laplace_centred(gpu_backend, shape, name):
    C.check_laplace_centred(gpu_backend, shape, name)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_laplace_staggered(gpu_backend, shape, name):
    C.check_laplace_staggered(gpu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_gradient_centred(gpu_backend, shape, name):
    C.check_gradient(gpu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_divergence_centred(gpu_backend, shape, name):
    C.check_divergence(gpu_backend, shape, name)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_curl_staggered(gpu_backend, shape, name):
    C.check_curl_staggered(gpu_backend, shape, name)


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_curl_centred(gpu_backend, shape, name):
    C.check_curl_centred(gpu_backend, shape, name)


def test_hand_values(gpu_backend):
    C.check_hand_values(gpu_backend)


@pytest.mark.parametrize("op", ['laplace', 'laplace_axes', 'laplace_vector', 'gradient', 'divergence'])
@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_backward_centred(gpu_backend, shape, name, op):
    C.check_backward(gpu_backend, shape, name, op)


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_backward_laplace_staggered(gpu_backend, shape, name):
    C.check_backward(gpu_backend, shape, name, 'laplace_staggered')


@pytest.mark.parametrize("name", C.STAGGERED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_backward_curl_staggered(gpu_backend, shape, name):
    C.check_backward(gpu_backend, shape, name, 'curl_staggered')


@pytest.mark.parametrize("name", C.CENTRED_EXTS)
@pytest.mark.parametrize("shape", C.SHAPES_2D)
def test_backward_curl_centred(gpu_backend, shape, name):
    C.check_backward(gpu_backend, shape, name, 'curl_centred')


def test_backward_entries_accumulate(gpu_backend):
    C.check_backward_accumulates(gpu_backend)


@pytest.mark.parametrize("chunk", [2, 3])
def test_marching_carries_planes_and_rows_in_registers(gpu_backend, chunk):
    C.check_marching_chunks(gpu_backend, chunk)


def test_gray_scott_step_replays_the_eager_bits(gpu_backend):
    with precision(32):
        u0, v0 = C.gray_scott_fields(64, gpu_backend, 32)
        step = jit_compile(lambda u, v: C.gray_scott(u, v, dt=0.5, **C.MAZE))
        ue, ve, uj, vj = u0, v0, u0, v0
        for _ in range(4):       # the capture and 3 replays
            ue, ve = C.gray_scott(ue, ve, dt=0.5, **C.MAZE)
            uj, vj = step(uj, vj)
            assert np.array_equal(ue.numpy(), uj.numpy()) and np.array_equal(ve.numpy(), vj.numpy())
        ug = CenteredGrid(u0.values[0].clone().requires_grad_(True), PERIODIC, x=64, y=64, backend=gpu_backend)
        with pytest.raises(NotImplementedError):
            step(ug, v0)

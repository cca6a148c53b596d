"""
The method-of-lines step on the MI355X (csrc/momentum.hpp: advect.differential forward and backward; diffuse.differential and
fluid.incompressible_rk4 over the kernels that exist): the checks of tests/momentum_cases.py on the device, plus the two accuracy facts of the step
(the energy error of the Taylor-Green decay and the temporal order), which the emulation is too slow for.
"""
import pytest

import momentum_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,name", C.FORWARD_CASES)
def test_forward_staggered(gpu_backend, shape, name):
    C.check_forward_staggered(gpu_backend, shape, name)


@pytest.mark.parametrize("shape,name", C.CENTRED_CASES)
def test_forward_centred(gpu_backend, shape, name):
    C.check_forward_centred(gpu_backend, shape, name)


def test_unaligned_buffers_give_the_same_bits(gpu_backend):
    C.check_unaligned(gpu_backend)


def test_nan_reaches_what_the_restatement_says(gpu_backend):
    C.check_nan_reach(gpu_backend)


@pytest.mark.parametrize("chunk", [2, 3])
def test_marching_carries_planes_in_registers(gpu_backend, chunk):
    C.check_marching_chunks(gpu_backend, chunk)


def test_hand_values(gpu_backend):
    C.check_hand_values(gpu_backend)


def test_storage_facts(gpu_backend):
    C.check_storage_facts(gpu_backend)


@pytest.mark.parametrize("shape,name", C.FORWARD_CASES)
def test_backward_staggered(gpu_backend, shape, name):
    C.check_backward(gpu_backend, shape, name, 'staggered')


@pytest.mark.parametrize("shape,name", C.CENTRED_CASES)
def test_backward_centred(gpu_backend, shape, name):
    C.check_backward(gpu_backend, shape, name, 'centred')


def test_backward_entries_accumulate(gpu_backend):
    C.check_backward_accumulates(gpu_backend)


def test_diffuse_differential(gpu_backend):
    C.check_diffuse_differential(gpu_backend)


@pytest.mark.parametrize("case", list(C.RK4_CASES))
def test_rk4_step_is_the_restatement(gpu_backend, case):
    C.check_rk4(gpu_backend, case)


def test_rk4_energy_error_and_temporal_order(gpu_backend):
    C.check_rk4_accuracy(gpu_backend)


def test_rk4_fp32(gpu_backend):
    C.check_rk4_fp32(gpu_backend)


def test_rk4_step_under_jit_compile(gpu_backend):
    C.check_rk4_jit(gpu_backend)


def test_gradient_through_an_rk4_step(gpu_backend):
    C.check_rk4_gradient(gpu_backend)


def test_refusals_name_the_way_out(gpu_backend):
    for label, call, word in C.refusal_cases(gpu_backend):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert word in str(e.value), (label, str(e.value))

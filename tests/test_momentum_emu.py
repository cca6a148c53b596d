"""
The method-of-lines step (advect.differential / diffuse.differential / fluid.incompressible_rk4; csrc/momentum.hpp) on the emulation
library: the pins of the float64 restatement (pure NumPy), element-wise forward and backward parity, hand values, storage facts, the RK4 step against
the restatement, jit_compile, the gradient through a step and the refusals. The accuracy facts of the step on the package run on the device only
(tests/test_gpu_momentum.py): the emulation takes too long for them.
"""
import numpy as np
import pytest

import momentum_cases as C
import momentum_ref as M

O = M.O


# ---- 1. the reference is pinned (pure NumPy) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", C.FORWARD_CASES)
def test_restatement_is_the_oracle_composition(shape, name):
    """ -(v . grad) u written out with index gathers == the composition of oracle.pad_component and oracle.component_at_faces, to 1e-14 relative """
    dom = C.domain(name, shape)
    for B in (1, 3):
        rng = C.rng_for('pin', shape, name, B)
        u, v = C._faces(shape, name, B, np.float64, rng), C._faces(shape, name, B, np.float64, rng)
        for a, b in ((u, v), (u, u)):
            got, S = M.advect_staggered(a, b, dom)
            want = M.advect_staggered_oracle(a, b, dom)
            for g, w, s in zip(got, want, S):
                assert np.abs(g - w).max() <= 1e-14 * max(np.abs(w).max(), 1e-300)
                assert (np.abs(g) <= s * (1 + 1e-12)).all()          # S bounds the value term by term


def test_restatement_energy_error_of_the_taylor_green_decay():
    """ E(T) / E(0) against exp(-4 nu T), nu = 0.1, T = 0.8, dt = 0.1: +0.41 % at 16^2, +0.103 % at 32^2 (second order in space), within a quarter """
    def run(n, dt, steps):
        dom = M.periodic_domain((n, n))
        return M.rk4_run(M.taylor_green(dom), np.zeros((1, n, n)), dt, steps, 0.1, dom)[0]
    for n, fact in C.ENERGY_FACTS.items():
        err = C.energy_error(run, n)
        assert 0 < err <= 1.25 * fact, (n, err)
    # ... and hardly any dependence on dt
    assert abs(C.energy_error(lambda n, dt, steps: run(n, 0.2, 4), 16) - C.energy_error(lambda n, dt, steps: run(n, 0.05, 16), 16)) < 2e-4


def test_restatement_is_third_order_in_time():
    """ halving dt through 0.1 -> 0.05 -> 0.025 divides the velocity error by more than 6 (second order would give 4; the restatement gives 8.2 and 8.2): the
    velocity is third order, not fourth, because of the way the stages update the pressure -- the reference's algorithm """
    dom = M.periodic_domain((16, 16))
    v0, p0 = M.taylor_green(dom, perturbed=True), np.zeros((1, 16, 16))
    r1, r2 = C.order_ratios(lambda dt, steps: M.rk4_run(v0, p0, dt, steps, 0.1, dom)[0])
    assert r1 >= 6 and r2 >= 6, (r1, r2)


def test_rk4_tolerances_come_from_the_restatement_alone():
    C.check_rk4_reference_spread()


def test_torch_and_numpy_forms_of_the_centred_restatement_agree_with_a_plain_loop():
    """ the centred formula once more, as explicit Python loops over the cells of a small grid """
    rng = np.random.default_rng(3)
    shape, dx = (4, 5), (0.3, 0.5)
    codes, consts = [[O.CLOSED, O.OPEN], [O.PERIODIC, O.PERIODIC]], [(0.7, 0.0), (0.0, 0.0)]
    u, v = rng.standard_normal((1, 2) + shape), rng.standard_normal((1, 2) + shape)
    ref, _ = M.advect_centered(u, v, dx, codes, consts)

    def tap(c, i, j):
        if i < 0:
            return 0.7
        i = min(i, shape[0] - 1)
        return u[0, c, i, j % shape[1]]
    for c in range(2):
        for i in range(shape[0]):
            for j in range(shape[1]):
                want = -(v[0, 0, i, j] * (tap(c, i + 1, j) - tap(c, i - 1, j)) / (2 * dx[0]) + v[0, 1, i, j] * (tap(c, i, j + 1) - tap(c, i, j - 1)) / (2 * dx[1]))
                assert abs(ref[0, c, i, j] - want) <= 1e-13


# ---- 2. forward, element by element -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", C.FORWARD_CASES)
def test_forward_staggered(emu_backend, shape, name):
    C.check_forward_staggered(emu_backend, shape, name)


@pytest.mark.parametrize("shape,name", C.CENTRED_CASES)
def test_forward_centred(emu_backend, shape, name):
    C.check_forward_centred(emu_backend, shape, name)


def test_unaligned_buffers_give_the_same_bits(emu_backend):
    C.check_unaligned(emu_backend)


def test_nan_reaches_what_the_restatement_says(emu_backend):
    C.check_nan_reach(emu_backend)


@pytest.mark.parametrize("chunk", [2, 3])
def test_marching_carries_planes_in_registers(emu_backend, chunk):
    C.check_marching_chunks(emu_backend, chunk)


# ---- 3. hand values and storage facts -----------------------------------------------------------------------------------------------------------
def test_hand_values(emu_backend):
    C.check_hand_values(emu_backend)


def test_storage_facts(emu_backend):
    C.check_storage_facts(emu_backend)


# ---- 4. backward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name", C.FORWARD_CASES)
def test_backward_staggered(emu_backend, shape, name):
    C.check_backward(emu_backend, shape, name, 'staggered')


@pytest.mark.parametrize("shape,name", C.CENTRED_CASES)
def test_backward_centred(emu_backend, shape, name):
    C.check_backward(emu_backend, shape, name, 'centred')


def test_backward_entries_accumulate(emu_backend):
    C.check_backward_accumulates(emu_backend)


# ---- 5. diffuse.differential ----------------------------------------------------------------------------------------------------------------------
def test_diffuse_differential(emu_backend):
    C.check_diffuse_differential(emu_backend)


# ---- 6. incompressible_rk4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.RK4_CASES))
def test_rk4_step_is_the_restatement(emu_backend, case):
    C.check_rk4(emu_backend, case)


def test_rk4_fp32(emu_backend):
    C.check_rk4_fp32(emu_backend)


def test_rk4_step_under_jit_compile(emu_backend):
    C.check_rk4_jit(emu_backend)


def test_gradient_through_an_rk4_step(emu_backend):
    C.check_rk4_gradient(emu_backend)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_way_out(emu_backend):
    for label, call, word in C.refusal_cases(emu_backend):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert word in str(e.value), (label, str(e.value))

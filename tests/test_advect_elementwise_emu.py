"""
Element-wise parity of the forward advection passes under the CPU emulation (tests/hipemu), in fp32 and fp64: every output sample of every forward advection entry
point, on every path (adaptive reach, fixed reach 1 / 2, gather kernels, LDS-DMA and register-staged fills, 2-D windows, several chunks with a ragged last one),
against the float64 restatement of the oracle (tests/adjoint_ref.py) under a per-sample bound -- tests/advect_forward_cases.py describes the rule. Each check
asserts, inside the functions it calls, finiteness, the pin of the restatement to the oracle's float64 forward (<= 1e-12), the per-sample bound, the cap on
samples that admit more than one limiter window and the path that ran. tests/test_gpu_advect_elementwise.py repeats the cases on the device. Every case prints
its figures.
"""
import numpy as np
import pytest

import adjoint_cases as A
import advect_forward_cases as F
import parity_cases as pc

MEM = pc.NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
_id = F.case_id
THREE_PATHS = ("adaptive", "halo 1", "halo 0")
# the grading along the slowest axis, and walls at rest, on a few grids only: they differ from their siblings in the inputs, not in the code they reach
GRADED = [(c, "graded fast") for c in F.CASES] + [(F.CASES[k], "graded slow") for k in (4, 5, 10)]
NEAR_REST = [(c, "rest walls") for c in F.CASES] + [(F.CASES[k], "rest") for k in (0, 4, 8, 11)]
SMALL = A.SMALL_CASES[::2]
_id2 = lambda ck: f"{F.case_id(ck[0])}-{ck[1].replace(' ', '_')}"


@DTYPES
@pytest.mark.parametrize("dt", [0.7, 2.9], ids=["cfl<1", "cfl3"])
@pytest.mark.parametrize("case", F.CASES, ids=_id)
def test_random_fields_on_every_path(emu_ctx, case, dt, dtype):
    """ white noise; dt 0.7: every displacement below one cell, dt 2.9: CFL about 3 (fix-up list, reach 2) """
    res, bc, batch = case
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, dt, "random", seed=1)


@DTYPES
@pytest.mark.parametrize("case_kind", GRADED, ids=_id2)
def test_graded_fields_small_samples_matter(emu_ctx, case_kind, dtype):
    """ fields times exp(-18 x / L) along the fast (slowest) axis: nine decades; the bound of a sample scales with the sample's own taps """
    (res, bc, batch), kind = case_kind
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, 0.7, kind, seed=2, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case_kind", NEAR_REST, ids=_id2)
def test_fields_near_rest_window_follows_the_sign(emu_ctx, case_kind, dtype):
    """ displacements of about 3e-8 cells of either sign, walls at rest and walls moving at up to 0.5: the limiter window follows the sign of the displacement
    (absolute coordinates in fp32 lose it), the interpolation weight next to a moving wall carries eps / 2 cells -- covered by the envelope, not by an exemption """
    (res, bc, batch), kind = case_kind
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, 2.9, kind, seed=3, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case", F.CASES[:6] + F.CASES[9:10], ids=_id)
def test_kinks_on_purpose_exempt_from_the_window_cap(emu_ctx, case, dtype):
    """ velocities dx / dt (k + r), r exactly 0 or 1/2: backward lookups land exactly on cell boundaries and on the staggered window's half-cell kink; both windows
    are admissible by construction (no cap), the value must stay within the bound of one of them """
    res, bc, batch = case
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, 0.7, "kinks (exempt from the window cap)", seed=4, strengths=(1.0,), only_paths=THREE_PATHS)


@DTYPES
@pytest.mark.parametrize("case", SMALL, ids=A.case_id)
def test_axes_of_one_to_three_cells(emu_ctx, case, dtype):
    """ axes of 1, 2 and 3 cells under every boundary kind that stores faces, as first, middle and last axis: lookups that wrap or clamp several times """
    res, bc, batch = case
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, 2.9, "random", seed=5, strengths=(0.6,), only_paths=THREE_PATHS)
    F.run_case(emu_ctx, MEM, res, bc, dtype, batch, 0.7, "rest walls", seed=6, strengths=(1.0,), only_paths=("adaptive", "halo 0"))


@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-batch", "shared"])
@pytest.mark.parametrize("case", F.GRID_SAMPLE_CASES, ids=_id)
def test_grid_sample_value_min_max(emu_ctx, case, shared, dtype):
    """ phihip_grid_sample: the value under the per-sample bound, out_min / out_max equal to the reference's taps exactly """
    F.run_grid_sample(emu_ctx, MEM, case[0], case[1], dtype, shared)


@DTYPES
def test_hand_derived_limiter_table(emu_ctx, dtype):
    """ fwd, bwd, window and limited result against literals worked out by hand (tests/limiter_table.py), not through the oracle: equality """
    F.check_limiter_table(emu_ctx, MEM, dtype)


def test_bound_rejects_the_fp32_oracle_on_rows_of_134_cells():
    """ tightness canary, measured on the reference alone: the fp32 oracle (absolute coordinates in fp32) must itself exceed the kernels' bound on (5, 6, 134); a
    bound it passed could not tell the kernels' displacement-relative lookup from the arithmetic it replaced """
    res, bc, batch = F.CANARY_CASE
    for dt in (0.7, 2.9):
        worst = F.oracle32_worst_ratio(res, bc, dt, "random", seed=1, batch=batch)
        print("advect-elementwise canary", res, dt, worst)
        assert all(r > 1.0 for r in worst.values()), worst


def test_near_rest_oracle32_picks_wrong_windows_where_the_reference_does_not():
    """ the property the kernels have and the fp32 oracle lacks, stated on the reference: near rest the float64 evaluation leaves no sample with two admissible
    windows (the sign of the displacement decides), while the fp32 oracle is beyond the bound in part of the samples """
    res, bc, batch = F.CASES[0]
    dom, grid, v, f, s, s_codes, s_consts, rng = F.make_inputs(res, bc, np.float32, batch, 2.9, "rest walls", 3)
    (e,) = F.expect_mac_cormack_centered(s, v, 2.9, dom, np.float32, s_codes, s_consts, 1.0)
    assert not e.multi.any()
    wrong = int((e.ratio(e.oracle32) > 1).sum())
    print("advect-elementwise near rest: fp32 oracle beyond the bound in", wrong, "of", e.ref.size)
    assert wrong > 0

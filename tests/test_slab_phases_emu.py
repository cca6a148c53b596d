"""
Element-wise parity of the slab-decomposed CG phases under the CPU emulation (tests/hipemu): phihip_slab_residual, phihip_slab_matvec, phihip_slab_update and
phihip_slab_state with the neighbours' planes as halos, every output element and every sum against the float64 reference on the undivided grid --
tests/slab_phase_cases.py describes the harness and the rule. The emulation runs a subset (its fibres are slow): the three-rank chain in fp32 and fp64 with
flags, one plain case per row width, the negative controls. tests/test_gpu_slab_phases.py runs every case on the device. Every case prints its figures.
"""
import numpy as np
import pytest

import parity_cases as pc
import slab_phase_cases as S

MEM = pc.NumpyMem()
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def ranks(emu_library):
    """ one context per emulated rank: the control block and slab_cur are per context """
    from phiflow_amd import _capi
    ctxs = [_capi.Context(emu_library, 0) for _ in range(3)]
    for c in ctxs:
        c.set_autotune(False)
    yield ctxs
    for c in ctxs:
        c.close()


# ---- the tables and the restated control block (NumPy only) ---------------------------------------------------------------------------------------------------------
def test_the_width_cases_reach_every_row_path():
    assert [S.march_vector_width(res[-1], S.DT[name]) for name, res, force in S.WIDTH_CASES] == S.WIDTH_VECS
    assert 8 in S.available_tiles(264, np.float32) and S.TILE_SHAPES[8] == (1, 128) and S.TILE_SHAPES[0] == (1, 16)
    assert S.UNEVEN7 == [0, 3, 5, 7]
    for name, res, cuts, (tid, chunk) in S.TILE_CASES:
        V = 4 if name == "f32" else 2
        assert tid in S.available_tiles(res[-1], S.DT[name])
        assert any(b1 - b0 > chunk for b0, b1 in zip(cuts, cuts[1:]))                    # a slab cut into several chunks
    assert any(-(-res[1] // 16) >= 2 and -(-res[2] // (16 * (4 if name == "f32" else 2))) >= 2 for name, res, cuts, force in S.TILE_CASES)
    assert {S._bc(k)[0] for k in range(3)} == set(S.SLAB_BCS)


def test_the_restated_control_block():
    solve = pc.C.Solve(1e-3, 0.5, 2, 0, 0, 0)
    s = S.advance("first", {}, 4.0, 100.0, solve)
    assert (s["tol_sq"], s["converged"], s["cont"], s["iterations"]) == (0.25, 0, 1, 0)
    s = S.advance("alpha", s, -8.0, 0.0, solve)
    assert (s["alpha"], s["iterations"]) == (-0.5, 1)
    s = S.advance("beta", s, 1.0, 0.0, solve)
    assert (s["beta"], s["rsq"], s["cont"]) == (0.25, 1.0, 1)
    s = S.advance("beta", S.advance("alpha", s, 2.0, 0.0, solve), 0.5, 0.0, solve)
    assert (s["iterations"], s["converged"], s["cont"]) == (2, 0, 0)                      # max_iterations reached
    frozen = S.advance("alpha", s, 1.0, 0.0, solve)
    assert frozen == s
    assert S.advance("first", {}, float("nan"), 1.0, solve)["diverged"] == 1 and S.advance("first", {}, 0.2, 1.0, solve)["converged"] == 1


@DTYPES
@pytest.mark.parametrize("tamper", S.TAMPERS)
def test_the_reference_alone_separates_the_wrong_inputs(dtype, tamper):
    sep = S.control_separation(dtype, tamper)
    print(f"slab-phases control {tamper} {np.dtype(dtype).name}: the reference moves by {sep:.3g} bounds")
    assert sep >= 100.0


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_chain_over_three_ranks_with_flags(ranks, dtype):
    """ one-plane and two-plane slabs, a periodic slab axis, flags across the cuts, entry 1 converged at the start, the peeks """
    res, cuts, k = S.CHAIN_CASES[0]
    S.run_chain(ranks, MEM, res, S._bc(k), dtype, cuts, flags=True, seed=1)


@pytest.mark.parametrize("k", range(len(S.WIDTH_CASES)), ids=lambda k: f"{S.WIDTH_CASES[k][0]}-n2={S.WIDTH_CASES[k][1][-1]}")
def test_one_plain_case_per_row_width(ranks, k):
    name, res, force = S.WIDTH_CASES[k]
    S.run_phases(ranks, MEM, res, S._bc(k), S.DT[name], [0, 1, 3, res[0]], kinds=("random",), flags=(False,), seed=2 + k, force=force)


@DTYPES
def test_negative_controls(ranks, dtype):
    counts = S.control_counts(ranks, MEM, dtype, seed=3)
    print(f"slab-phases controls {np.dtype(dtype).name}: violations {counts}")
    assert counts[None] == 0
    for tamper in S.TAMPERS:
        assert counts[tamper] > 0, tamper

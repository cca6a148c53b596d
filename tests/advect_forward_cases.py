"""
Element-wise parity of the FORWARD advection passes (phiflow_amd/csrc/advect_tile.hip, advect_win.hip, the gather kernels of advect.hip, advect_cvec.hpp),
in fp32 and fp64, on every path. Used by tests/test_advect_elementwise_emu.py (emulation), tests/test_gpu_advect_elementwise.py (MI355X) and
tests/fuzz_parity.py. DESIGN.md "f11" holds the derivation of the constants below.

Reference: the float64 torch forward functions of tests/adjoint_ref.py on the inputs AFTER rounding to the element type, pinned to the oracle's float64
forward in every case (adjoint_ref.pin; advect_centered_vector: tests/centered_vector_ref.py).

Rule for an interpolated value, per sample, everything computed by the reference in float64:
        |kernel - ref| <= K eps S + E
    S = sum_k w_k |t_k|             the same lookup applied to |field| with |constants|
    E = max over sigma in {-1,0,1}^D of |ref(c + sigma * delta_frac) - ref(c)|          the coordinate envelope
        + eps / 2 * G,  G = sum over lerp_cell's levels and tap pairs of w_rest f |hi - lo|: the rounded difference hi - lo of a pair perturbs THAT pair's
                        fraction by eps / 2 f, every pair with its own sign (adjoint_ref.lerp_difference_scale; phihip_grid_sample sums weights: no such term)
    delta_floor[a] = K_DISP eps M_a + delta_ref[a]      M_a = |dt| / dx_a * (the kernel's mean of the |velocity| samples it averages): the sum of the
                                                        magnitudes of the displacement's terms in index units; decides the cell and the limiter window
    delta_frac[a]  = delta_floor[a] + eps / 2           frac_part
    delta_ref[a]   = 8 eps(float64) (n_a + 1 + M_a)     the reference's own absolute float64 coordinate
MacCormack: clip(new, lo, hi), new = fma(ch, field - bwd, fwd). The bound of `fwd` enters the second lookup through the largest bound among its taps; clip is
1-Lipschitz in `new`; lo / hi are exact taps of the window. The window is the only discrete decision: a sample whose limiter coordinate lies within
delta_floor (own axis of a staggered component: + eps / 2 (M + 1/2), the rounded half-cell shift) of an integer admits the windows on both sides and passes
if it is within its bound of the clamp under ANY admissible window. The reference takes that distance from the DISPLACEMENT (Lookup.limiter), like the kernels:
near rest a point lies 1e-8 +- 1e-14 cells from a sample, which an absolute float64 coordinate on an axis of 131 cells cannot place. No sample is dropped. The share of samples with more than one admissible window is capped:
<= 5e-4 per output array, zero on arrays of fewer than 2 000 samples, zero in fp64 -- the reference alone picks the seed (first of seed + 1000 k).
"""
import numpy as np
import torch

import adjoint_ref as R
import centered_vector_ref as CV
from parity_cases import CLO, OPN, PER, C, O, advect_tol, make_case

RECORDS = []          # one dict per (entry point, path): printed by `report()`, the source of the tables in DESIGN.md
K_LERP = 2.0          # lerp_cell: one fma rounding per axis, D / 2 eps <= 1.5 eps of S, rounded up
K_WEIGHTS = 6.0       # gather_multilinear_weights (phihip_grid_sample): 1 - f, D - 1 weight products, value * weight, 2^D - 1 additions: 11 eps / 2, rounded up
K_DISP = 4.0          # displacement: sum4_chain (3 additions of magnitudes) + (T)dt (T)rdx, their product, the product with the mean: 7 eps / 2, rounded up
K_REF = 8.0           # the reference's own float64 evaluation, in eps(float64) of S
WINDOW_CAP = 5e-4
SEED_TRIES = 6


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


EPS64 = eps_of(np.float64)


def report():
    for r in RECORDS:
        print("advect-elementwise", " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()), flush=True)


def _t(a):
    return R.tensor(a, torch.float64)


def _tl(arrays):
    return [_t(a) for a in arrays]


def _np(t):
    return t.detach().numpy().astype(np.float64)


def _abs_dom(dom):
    return O.Domain(dom.res, dom.lower, dom.upper, dom.bc, np.abs(dom.bc_val))


class Expected:
    """ what the reference says about one output array """
    def __init__(self, ref, bound, oracle32, new=None, windows=None, multi=None):
        self.ref, self.bound, self.oracle32 = ref, bound, oracle32
        self.new, self.windows, self.multi = new, windows, multi

    @property
    def multi_share(self):
        return 0.0 if self.multi is None else float(self.multi.mean())

    def distance(self, got):
        """ |got - expected| per sample; MacCormack: the smallest distance over the admissible windows """
        got = got.astype(np.float64)
        if self.windows is None:
            return np.abs(got - self.ref)
        d = np.full(got.shape, np.inf)
        for lo, hi in self.windows:
            d = np.minimum(d, np.abs(got - np.clip(self.new, lo, hi)))
        return d

    def ratio(self, got):
        d = self.distance(got)
        return np.where(self.bound > 0, d / np.maximum(self.bound, 1e-300), np.where(d > 0, np.inf, 0.0))


def cap_ok(expected, dtype, exempt=False):
    """ the conditions that keep the window rule from hiding a failure """
    if exempt:
        return True
    for e in expected:
        if e.multi is None:
            continue
        n = int(e.multi.sum())
        if n and (np.dtype(dtype) == np.float64 or e.multi.size < 2000 or n > WINDOW_CAP * e.multi.size):
            return False
    return True


# ---- the reference: lookups, their deltas, bounds -------------------------------------------------------------------------------------------------------------
class Lookup:
    """ coordinates of a lookup (index units of the array looked up in) with the kernel's coordinate errors """
    def __init__(self, coords, mags, shape, dtype, own=None):
        eps = eps_of(dtype)
        self.coords = coords
        self.d_floor = [K_DISP * eps * m + K_REF * EPS64 * (n + 1.0 + m) for m, n in zip(mags, shape)]
        self.d_frac = [d + 0.5 * eps for d in self.d_floor]
        self.mags, self.own, self.eps = mags, own, eps

    def limiter(self, disp, shift_own=0.0):
        """ the limiter's cell and the point's distances from its ends, from the displacement `disp` (index units, float64) and the half-cell shift of a staggered
        component's own axis; delta: K_DISP eps M + the float64 error of `disp` + on the own axis the rounded shift """
        D = len(disp)
        shape = disp[0].shape
        base, below, above, delta = [], [], [], []
        for a in range(D):
            idx = torch.arange(shape[a + 1], dtype=torch.float64).reshape([-1 if k == a + 1 else 1 for k in range(D + 1)])
            own = a == self.own
            t = disp[a] + (shift_own if own else 0.0)
            fl = torch.floor(t)
            base.append(idx + fl)
            below.append(t - fl)
            above.append((fl + 1.0) - t)
            delta.append(K_DISP * self.eps * self.mags[a] + 4.0 * EPS64 * (1.0 + self.mags[a]) + (0.5 * self.eps * (self.mags[a] + 0.5) if own else 0.0))
        return base, below, above, delta


def interp(a, look, codes, consts, K, dtype):
    """ (value, bound) of the multilinear lookup of `a` at `look` """
    val = R.grid_sample(a, look.coords, codes, consts)
    S = R.grid_sample_scale(a, look.coords, codes, consts)
    E = R.grid_sample_envelope(a, look.coords, codes, consts, look.d_frac) + 0.5 * eps_of(dtype) * R.lerp_difference_scale(a, look.coords, codes, consts)
    return val, (K * eps_of(dtype) + K_REF * EPS64) * S + E


def mac_cormack(field, fwd_look, bwd_look, limiter, codes, consts, strength, dtype, pinned, abs_coords):
    """ (result, bound, new, windows, multi) of the limited MacCormack value for one array. fwd_look: the BACKWARD trace (the semi-Lagrangian lookup into the
    field), bwd_look: the forward trace (the lookup into fwd_adv). """
    eps = eps_of(dtype)
    ch = 0.5 * strength
    fwd, b_fwd = interp(field, fwd_look, codes, consts, K_LERP, dtype)
    bwd, b_own = interp(fwd, bwd_look, codes, consts, K_LERP, dtype)
    zero = [(0.0, 0.0)] * len(consts)
    b_taps = R.closest_limits(b_fwd, bwd_look.coords, codes, zero)[1]       # the largest bound among the taps (a constant tap carries none)
    b_bwd = b_taps + b_own
    new = fwd + ch * (field - bwd)
    # fma(ch, field - bwd, fwd): the difference, (T)ch and the fma round once each
    b_new = b_fwd + abs(ch) * b_bwd + eps * abs(ch) * (field - bwd).abs() + 0.5 * eps * new.abs() + K_REF * EPS64 * (fwd.abs() + (field - bwd).abs())
    windows, multi = R.limit_windows_cells(field, *limiter[:3], codes, consts, limiter[3])
    lo, hi = windows[0]
    res = torch.where(new < lo, lo, torch.where(new > hi, hi, new))
    # the window from the displacement gives the pinned restatement's result, except where ITS absolute float64 coordinate cannot place the point
    far = torch.ones(res.shape, dtype=torch.bool)
    for dist, n, m in zip(R.coord_distance(abs_coords), field.shape[1:], fwd_look.mags):
        far = far & (dist > K_REF * EPS64 * (n + 1.0 + m))
    off = ((res - pinned).abs() > 1e-12 * max(float(pinned.abs().max()), 1e-300)) & far
    assert not bool(off.any()), f"the limiter window taken from the displacement disagrees with the pinned restatement in {int(off.sum())} samples"
    return res, b_new, new, windows, multi


def _stag_lookups(v64, d, dt, dom, dtype):
    """ backward and forward lookups of the stored faces of component d, and the limiter's cells (cell frame: half a cell off along d) """
    D = dom.rank
    adom = _abs_dom(dom)
    va = [a.abs() for a in v64]
    mags = [(va[d] if c == d else R.component_at_faces(va, c, d, adom)) * (abs(dt) / dom.dx[c]) for c in range(D)]
    disp = [(v64[d] if c == d else R.component_at_faces(v64, c, d, dom)) * (-dt / dom.dx[c]) for c in range(D)]
    shape = dom.comp_shape(d)
    p_bwd, p_fwd = R._face_lookups(v64, d, -dt, dom, v64[d]), R._face_lookups(v64, d, dt, dom, v64[d])
    bwd = Lookup(R._index_coords(p_bwd, d, dom), mags, shape, dtype, own=d)
    fwd = Lookup(R._index_coords(p_fwd, d, dom), mags, shape, dtype, own=d)
    return bwd, fwd, bwd.limiter(disp, dom.face_offset(d) - 0.5)


def _cen_lookups(v64, dt, dom, dtype, like):
    D = dom.rank
    adom = _abs_dom(dom)
    ua = R.staggered_at_centers([a.abs() for a in v64], adom)
    u = R.staggered_at_centers(v64, dom)
    mags = [ua[c] * (abs(dt) / dom.dx[c]) for c in range(D)]
    bwd = Lookup(R._cell_frame(R._centre_lookups(v64, -dt, dom, like), dom), mags, dom.res, dtype)
    fwd = Lookup(R._cell_frame(R._centre_lookups(v64, dt, dom, like), dom), mags, dom.res, dtype)
    return bwd, fwd, bwd.limiter([u[c] * (-dt / dom.dx[c]) for c in range(D)])


def _to64(arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def expect_advect_staggered(f, v, dt, dom, dtype):
    f64, v64 = _tl(f), _tl(v)
    with torch.no_grad():
        R.pin(R.semi_lagrangian_staggered(f64, v64, dt, dom), O.semi_lagrangian_staggered(_to64(f), _to64(v), dt, dom), "semi_lagrangian_staggered")
        o32 = O.semi_lagrangian_staggered(f, v, dt, dom)
        out = []
        for d in range(dom.rank):
            codes, consts = R._comp_rule(dom, d)
            bwd, _, _ = _stag_lookups(v64, d, dt, dom, dtype)
            val, b = interp(f64[d], bwd, codes, consts, K_LERP, dtype)
            out.append(Expected(_np(val), _np(b), o32[d].astype(np.float64)))
    return out


def expect_mac_cormack_staggered(f, v, dt, dom, dtype, strength):
    f64, v64 = _tl(f), _tl(v)
    with torch.no_grad():
        pinned = R.mac_cormack_staggered(f64, v64, dt, dom, strength)
        R.pin(pinned, O.mac_cormack_staggered(_to64(f), _to64(v), dt, dom, strength), "mac_cormack_staggered")
        o32 = O.mac_cormack_staggered(f, v, dt, dom, strength)
        out = []
        for d in range(dom.rank):
            codes, consts = R._comp_rule(dom, d)
            bwd, fwd, lim = _stag_lookups(v64, d, dt, dom, dtype)
            res, b, new, windows, multi = mac_cormack(f64[d], bwd, fwd, lim, codes, consts, strength, dtype, pinned[d],
                                                      R._cell_frame(R._face_lookups(v64, d, -dt, dom, v64[d]), dom))
            out.append(Expected(_np(res), _np(b), o32[d].astype(np.float64), _np(new), [(_np(lo), _np(hi)) for lo, hi in windows], multi.numpy()))
    return out


def expect_advect_centered(s, v, dt, dom, dtype, s_codes, s_consts):
    s64, v64 = _t(s), _tl(v)
    with torch.no_grad():
        R.pin(R.semi_lagrangian_centered(s64, v64, dt, dom, s_codes, s_consts), O.semi_lagrangian_centered(s.astype(np.float64), _to64(v), dt, dom, s_codes, s_consts),
              "semi_lagrangian_centered")
        bwd, _, _ = _cen_lookups(v64, dt, dom, dtype, s64)
        val, b = interp(s64, bwd, s_codes, s_consts, K_LERP, dtype)
    return [Expected(_np(val), _np(b), O.semi_lagrangian_centered(s, v, dt, dom, s_codes, s_consts).astype(np.float64))]


def expect_mac_cormack_centered(s, v, dt, dom, dtype, s_codes, s_consts, strength):
    s64, v64 = _t(s), _tl(v)
    with torch.no_grad():
        pinned = R.mac_cormack_centered(s64, v64, dt, dom, s_codes, s_consts, strength)
        R.pin(pinned, O.mac_cormack_centered(s.astype(np.float64), _to64(v), dt, dom, s_codes, s_consts, strength), "mac_cormack_centered")
        bwd, fwd, lim = _cen_lookups(v64, dt, dom, dtype, s64)
        res, b, new, windows, multi = mac_cormack(s64, bwd, fwd, lim, s_codes, s_consts, strength, dtype, pinned, bwd.coords)
    o32 = O.mac_cormack_centered(s, v, dt, dom, s_codes, s_consts, strength).astype(np.float64)
    return [Expected(_np(res), _np(b), o32, _np(new), [(_np(lo), _np(hi)) for lo, hi in windows], multi.numpy())]


def expect_advect_centered_vector(field, vel, dt, dom, dtype, codes, consts):
    """ field (B, Cn, *res), vel (B, D, *res): one Expected per field component (B, *res) """
    D = dom.rank
    truth = CV.semi_lagrangian(field.astype(np.float64), vel.astype(np.float64), dt, dom.res, dom.lower, dom.upper, codes, consts)
    o32 = np.asarray(CV.semi_lagrangian(field, vel, dt, dom.res, dom.lower, dom.upper, codes, consts), np.float64)     # (float64 arithmetic throughout: recorded, no canary)
    B = field.shape[0]
    with torch.no_grad():
        pts = [np.broadcast_to(p[None], (B,) + p.shape) for p in O.cell_positions(dom, np.float64)]
        back = [p - dt * vel[:, a].astype(np.float64) for a, p in enumerate(pts)]
        coords = _tl(CV.index_coords(back, dom.res, dom.lower, dom.upper))
        mags = [_t(np.abs(vel[:, a])) * (abs(dt) / dom.dx[a]) for a in range(D)]
        look = Lookup(coords, mags, dom.res, dtype)
        out = []
        for c in range(field.shape[1]):
            val, b = interp(_t(field[:, c]), look, codes, consts, K_LERP, dtype)
            R.pin(val, truth[:, c], "advect_centered_vector")
            out.append(Expected(_np(val), _np(b), o32[:, c]))
    return out


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------------------------------
def compare(entry, path, dtype, dom, got, expected, exempt=False):
    """ every output array of one run against its Expected: finiteness, the per-sample bound, the window cap """
    worst = share = old = worst_o32 = 0.0
    fail = None
    for k, (a, e) in enumerate(zip(got, expected)):
        assert a.shape == e.ref.shape, (entry, path, k, a.shape, e.ref.shape)
        if not a.size:
            continue
        assert np.isfinite(a).all(), f"{entry} [{path}] array {k}: non-finite values"
        ratio = e.ratio(a)
        worst = max(worst, float(ratio.max()))
        share = max(share, e.multi_share)
        worst_o32 = max(worst_o32, float(e.ratio(e.oracle32).max()))
        old = max(old, float((np.abs(a.astype(np.float64) - e.oracle32) > advect_tol(dtype, dom) * max(float(np.abs(e.oracle32).max()), 1e-30)).mean()))
        if fail is None and ratio.max() > 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            fail = (f"{entry} [{path}] {np.dtype(dtype).name} res {dom.res} bc {dom.bc}: array {k} at {i}: kernel {a[i]!r} vs reference {e.ref[i]!r}, "
                    f"{ratio[i]:.3g} x the bound {e.bound[i]:.3e}; {int((ratio > 1).sum())} of {ratio.size} samples beyond their bound")
    RECORDS.append(dict(entry=entry, path=path, dtype=np.dtype(dtype).name, res="x".join(str(n) for n in dom.res), ratio=worst, multi=share, old_rule=old,
                        oracle32=worst_o32))
    assert cap_ok(expected, dtype, exempt), f"{entry} [{path}]: {share:.2e} of the samples of an array admit more than one limiter window"
    assert fail is None, fail
    return worst


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def tiled(dom):
    return all(n >= 4 for d in range(dom.rank) for n in dom.comp_shape(d)) and all(n >= 4 for n in dom.res)


def make_inputs(res, bc, dtype, batch, dt, kind, seed):
    """ domain, grid, velocity, a second staggered field, a scalar with its rule. Walls that move on every closed side; scalar constants non-zero, the constant
    side below and above. """
    D = len(res)
    rng = np.random.default_rng(seed)
    dom0 = O.Domain(res, (0.0,) * D, tuple(float(n) for n in res), bc)
    closed = np.asarray([[bc[a][s] == CLO for s in range(2)] for a in range(D)])
    scale = 0.25
    if kind.startswith("kinks"):
        def vals(shape):
            return (dom0.dx[0] / dt) * (rng.integers(-2, 2, shape) + 0.5 * rng.integers(0, 2, shape))
        bcv = vals((D, 2, D)) * closed[:, :, None]
        v = [vals((batch,) + dom0.comp_shape(c)).astype(dtype) for c in range(D)]
    else:
        wall = 0.0 if kind == "rest" else 0.5
        bcv = rng.uniform(-wall, wall, (D, 2, D)) * closed[:, :, None]
        v = [(rng.standard_normal((batch,) + dom0.comp_shape(c)) * scale).astype(dtype) for c in range(D)]
        if kind.startswith("rest"):
            v = [a * dtype(3e-8 / (abs(dt) * scale)) for a in v]
    bcv = bcv.astype(np.float32).astype(np.float64)
    dom, grid = make_case(tuple(res), bc, dtype, batch, bc_val=bcv)
    f = [rng.standard_normal(a.shape).astype(dtype) for a in v]
    s = rng.standard_normal((batch,) + dom.res).astype(dtype)
    if kind.startswith("graded"):
        ax = D - 1 if kind == "graded fast" else 0
        def grade(a):
            n = a.shape[ax + 1]
            g = np.exp(-18.0 * np.arange(n) / n).reshape([n if k == ax + 1 else 1 for k in range(a.ndim)])
            return (a * g).astype(dtype)
        f, s = [grade(a) for a in f], grade(s)
    flip = bool(rng.integers(0, 2))
    s_codes = tuple((PER, PER) if lo == PER else ((OPN, CLO) if flip ^ (a % 2 == 0) else (CLO, OPN)) for a, (lo, hi) in enumerate(bc))
    s_consts = [(float(np.float32(rng.normal())), float(np.float32(0.25 + rng.normal()))) for _ in bc]
    return dom, grid, v, f, s, s_codes, s_consts, rng


# ---- paths ---------------------------------------------------------------------------------------------------------------------------------------------------
def expect_self_dma(dom, dtype):
    """ advect_tile.hip: the tiled self-advection of reach 1 fills its ring by LDS-DMA on 3-D grids whose rows hold two 16-byte vectors (whole ones where the
    fast axis is periodic) and whose other extents reach 4 """
    vv = 16 // np.dtype(dtype).itemsize
    if dom.rank != 3:
        return False
    for c in range(3):
        n = dom.comp_shape(c)
        if n[2] < 2 * vv or n[1] < 4 or n[0] < 4 or (dom.bc[2][0] == PER and n[2] % vv):
            return False
    return True


def expect_window_dma(dom, dtype):
    """ advect_win.hip: the correction pass of mac_cormack(v, v) fills its windows by LDS-DMA on regular grids: 3-D, no closed side, periodic fast axis with rows
    of whole 16-byte vectors """
    vv = 16 // np.dtype(dtype).itemsize
    return (dom.rank == 3 and tiled(dom) and not any(side == CLO for pair in dom.bc for side in pair) and dom.bc[2][0] == PER
            and all(dom.comp_shape(c)[2] % vv == 0 for c in range(3)))


def ragged_chunk(dom):
    """ planes per workgroup that make a workgroup march several chunks with a ragged last one (0: the slow axis is too short) """
    n0 = max(dom.comp_shape(c)[0] for c in range(dom.rank))
    for c in (5, 7, 4, 3):
        if n0 > c and n0 % c:
            return c
    return 0


class Path:
    def __init__(self, label, halo=-1, dma=1, chunk=0):
        self.label, self.halo, self.dma, self.chunk = label, halo, dma, chunk


def paths_for(dom, self_adv, reach2=True):
    out = [Path("adaptive"), Path("halo 1", 1), Path("halo 0", 0)]
    if reach2:
        out.insert(2, Path("halo 2", 2))
    if self_adv:
        out.insert(2, Path("halo 1 registers", 1, dma=0))
        if dom.rank == 3 and ragged_chunk(dom):
            out.append(Path(f"halo 1 chunk {ragged_chunk(dom)}", 1, chunk=ragged_chunk(dom)))
    return out


def run_paths(ctx, mem, dom, dtype, paths, launch, entry, expected, exempt=False, self_kind=None):
    """ `launch()` -> list of output handles, once per path; the settings are restored whatever happens. self_kind: 'tile' (advect_staggered(v, v)) or 'windows'
    (mac_cormack_staggered(v, v)): the LDS-DMA flag and the chunk length are asserted for those. """
    try:
        ctx.set_advect_windows_2d(True)
        for p in paths:
            ctx.set_advect_halo(p.halo)
            ctx.set_advect_dma(p.dma)
            ctx.set_advect_chunk(p.chunk)
            outs = launch()
            mem.sync()
            got = [mem.to_host(h) for h in outs]
            if p.halo == 1 and tiled(dom):
                redone, total = ctx.advect_fallback_stats()
                assert total > 0, f"{entry} [{p.label}]: no LDS-staged launch ran"
            if p.halo == 1 and self_kind and dom.rank == 3 and tiled(dom):
                want = bool(p.dma) and (expect_self_dma(dom, dtype) if self_kind == 'tile' else expect_window_dma(dom, dtype))
                ran = ctx.set_advect_dma(-1)
                assert ran == want, f"{entry} [{p.label}]: LDS-DMA kernel ran: {ran}, expected {want}"
                if p.chunk:
                    n0 = max(dom.comp_shape(c)[0] for c in range(3))
                    assert ctx.query_advect_chunk() == min(p.chunk, n0), f"{entry} [{p.label}]: chunk {ctx.query_advect_chunk()}"
            compare(entry, p.label, dtype, dom, got, expected, exempt)
    finally:
        ctx.set_advect_dma(1)
        ctx.set_advect_halo(-1)
        ctx.set_advect_chunk(0)
        ctx.set_advect_windows_2d(False)


# ---- the checks: one entry point on one case, every path -----------------------------------------------------------------------------------------------------------
def _P(mem, hs):
    return [mem.ptr(h) for h in hs]


def _pick(build, dtype, exempt, what):
    """ the first of SEED_TRIES seeds whose REFERENCE satisfies the window cap: build(attempt) -> (inputs, expected) """
    for attempt in range(SEED_TRIES):
        inputs, expected = build(attempt)
        if cap_ok(expected, dtype, exempt):
            return inputs, expected
    raise AssertionError(f"{what}: no seed of {SEED_TRIES} keeps the share of multi-window samples within the cap")


def check_entry(ctx, mem, entry, res, bc, dtype, batch=2, dt=0.7, kind="random", seed=0, strength=1.0, only_paths=None):
    """ entry: advect_staggered[self|other], advect_centered, mac_cormack_staggered[self|other], mac_cormack_centered, advect_centered_vector """
    exempt = kind.startswith("kinks")
    name, _, form = entry.partition("[")
    form = form.rstrip("]")

    def build(attempt):
        dom, grid, v, f, s, s_codes, s_consts, rng = make_inputs(res, bc, dtype, batch, dt, kind, seed + 1000 * attempt)
        fld = v if form == "self" else f
        if name == "advect_staggered":
            exp = expect_advect_staggered(fld, v, dt, dom, dtype)
        elif name == "mac_cormack_staggered":
            exp = expect_mac_cormack_staggered(fld, v, dt, dom, dtype, strength)
        elif name == "advect_centered":
            exp = expect_advect_centered(s, v, dt, dom, dtype, s_codes, s_consts)
        elif name == "mac_cormack_centered":
            exp = expect_mac_cormack_centered(s, v, dt, dom, dtype, s_codes, s_consts, strength)
        elif name == "advect_centered_vector":
            D = dom.rank
            vel = (rng.standard_normal((batch, D) + dom.res) * (3e-8 / abs(dt) if kind.startswith("rest") else 0.25)).astype(dtype)
            field = np.stack([s, s[::-1] * dtype(0.5)] + ([np.roll(s, 1, axis=-1) * dtype(2.0)] if D == 3 else []), axis=1).astype(dtype)
            exp = expect_advect_centered_vector(field, vel, dt, dom, dtype, s_codes, s_consts)
            return (dom, grid, v, fld, s, s_codes, s_consts, field, vel), exp
        else:
            raise ValueError(entry)
        return (dom, grid, v, fld, s, s_codes, s_consts, None, None), exp

    (dom, grid, v, fld, s, s_codes, s_consts, cfield, cvel), expected = _pick(build, dtype, exempt, entry)
    dv = [mem.to_dev(a) for a in v]
    what = f"{entry} {kind} dt={dt}" + (f" strength={strength}" if name.startswith("mac") else "")
    if name in ("advect_staggered", "mac_cormack_staggered"):
        df = dv if form == "self" else [mem.to_dev(a) for a in fld]

        def launch():
            out = [mem.empty(a.shape, dtype) for a in v]
            if name == "advect_staggered":
                ctx.advect_staggered(grid, _P(mem, df), _P(mem, dv), _P(mem, out), dt)
            else:
                ctx.mac_cormack_staggered(grid, _P(mem, df), _P(mem, dv), _P(mem, out), dt, strength)
            return out
        self_adv = form == "self"
        paths = paths_for(dom, self_adv, reach2=name == "advect_staggered") if self_adv else [Path("adaptive"), Path("halo 0", 0)]
        self_kind = None if not self_adv else ('tile' if name == "advect_staggered" else 'windows')
    elif name in ("advect_centered", "mac_cormack_centered"):
        ds = mem.to_dev(s)

        def launch():
            out = mem.empty(s.shape, dtype)
            if name == "advect_centered":
                ctx.advect_centered(grid, mem.ptr(ds), s_codes, s_consts, _P(mem, dv), mem.ptr(out), dt)
            else:
                ctx.mac_cormack_centered(grid, mem.ptr(ds), s_codes, s_consts, _P(mem, dv), mem.ptr(out), dt, strength)
            return [out]
        paths, self_kind = paths_for(dom, False), None
    else:
        dfield, dvel = mem.to_dev(cfield), mem.to_dev(cvel)

        def launch():
            out = mem.empty(cfield.shape, dtype)
            ctx.advect_centered_vector(grid, mem.ptr(dfield), cfield.shape[0], cfield.shape[1], s_codes, s_consts, mem.ptr(dvel), cvel.shape[0], mem.ptr(out), dt)
            return [out]
        paths, self_kind = [Path("adaptive"), Path("halo 0", 0)], None
    if only_paths is not None:
        paths = [p for p in paths if p.label.split(" chunk")[0] in only_paths]
    if name == "advect_centered_vector":
        inner = launch

        def launch():      # (B, Cn, *res) -> one array per component
            return [inner()[0][:, c] for c in range(cfield.shape[1])]
    run_paths(ctx, mem, dom, dtype, paths, launch, what, expected, exempt, self_kind)


ENTRIES = ("advect_staggered[self]", "advect_staggered[other]", "advect_centered", "mac_cormack_staggered[self]", "mac_cormack_staggered[other]",
           "mac_cormack_centered", "advect_centered_vector")


def run_case(ctx, mem, res, bc, dtype, batch=2, dt=0.7, kind="random", seed=0, entries=ENTRIES, strengths=(1.0, 0.6), only_paths=None):
    """ every entry point of `entries` on one case; prints the figures of the case (also when a check fails) """
    del RECORDS[:]
    try:
        for entry in entries:
            if entry.startswith("mac_cormack_staggered"):
                for st in strengths:
                    check_entry(ctx, mem, entry, res, bc, dtype, batch, dt, kind, seed, st, only_paths)
            else:
                check_entry(ctx, mem, entry, res, bc, dtype, batch, dt, kind, seed, 0.8 if entry == "mac_cormack_centered" else 1.0, only_paths)
    finally:
        report()


# ---- grid_sample ---------------------------------------------------------------------------------------------------------------------------------------------
def check_grid_sample(ctx, mem, shape, codes, dtype, batch=2, points=301, shared_values=False, seed=0, spread=2.5, graded=False):
    """ phihip_grid_sample with out, out_min, out_max: the coordinates are inputs (the reference splits the same numbers: delta_floor = 0, delta_frac = eps / 2 for
    coord - floor(coord)), so min and max are exact taps of ONE window and must equal the reference's exactly """
    D = len(shape)
    rng = np.random.default_rng(seed)
    eps = eps_of(dtype)
    consts = [(float(np.float32(rng.normal())), float(np.float32(rng.normal()))) for _ in shape]
    vb = 1 if shared_values else batch
    values = rng.standard_normal((vb,) + tuple(shape)).astype(dtype)
    if graded:
        n = shape[-1]
        values = (values * np.exp(-18.0 * np.arange(n) / n)).astype(dtype)
    coords = [((rng.random((batch, points)) * (2 * spread + 1) - spread) * n).astype(dtype) for n in shape]
    coords[0][:, :4] = np.asarray([0.0, -1.0, shape[0] - 1.0, float(shape[0])], dtype)[None]     # exactly on samples / one step outside
    coords[-1][:, 4:8] = np.asarray([-0.5, 0.5, shape[-1] - 0.5, -1e-9], dtype)[None]
    bc_val = [[[consts[a][s], 0.0, 0.0] for s in range(2)] for a in range(D)]
    grid = C.make_grid(D, C.PHIHIP_F64 if np.dtype(dtype) == np.float64 else C.PHIHIP_F32, batch, shape, (0.0,) * D, (1.0,) * D, codes, bc_val)
    dom = O.Domain(shape, (0.0,) * D, (1.0,) * D, codes)
    vals_b = np.array(np.broadcast_to(values.astype(np.float64), (batch,) + tuple(shape)))
    with torch.no_grad():
        a64, c64 = _t(vals_b), _tl(coords)
        ref = R.grid_sample(a64, c64, codes, consts)
        R.pin(ref, O.grid_sample(vals_b, _to64(coords), codes, consts), "grid_sample")
        S = R.grid_sample_scale(a64, c64, codes, consts)
        E = R.grid_sample_envelope(a64, c64, codes, consts, [0.5 * eps] * D)
        lo, hi, _ = R.closest_limits(a64, c64, codes, consts)
    o_lo, o_hi = O.closest_limits(vals_b, _to64(coords), codes, consts)
    assert np.array_equal(_np(lo), o_lo) and np.array_equal(_np(hi), o_hi), "closest_limits: the restatement differs from the oracle"
    o32 = O.grid_sample(np.broadcast_to(values, (batch,) + tuple(shape)), coords, codes, consts).astype(np.float64)
    expected = [Expected(_np(ref), _np((K_WEIGHTS * eps + K_REF * EPS64) * S + E), o32)]
    dvals, dc = mem.to_dev(values), [mem.to_dev(c) for c in coords]
    dout, dmin, dmax = (mem.empty((batch, points), dtype) for _ in range(3))
    ctx.grid_sample(grid, mem.ptr(dvals), vb, _P(mem, dc), points, mem.ptr(dout), mem.ptr(dmin), mem.ptr(dmax))
    mem.sync()
    for got, want, what in ((mem.to_host(dmin), _np(lo), "out_min"), (mem.to_host(dmax), _np(hi), "out_max")):
        assert np.isfinite(got).all(), f"grid_sample {what}: non-finite"
        assert np.array_equal(got.astype(np.float64), want), f"grid_sample {what}: {int((got.astype(np.float64) != want).sum())} of {want.size} taps differ from the reference's"
    compare("grid_sample" + (" shared values" if shared_values else "") + (" graded" if graded else ""), "-", dtype, dom, [mem.to_host(dout)], expected)


GRID_SAMPLE_CASES = [((6, 7), ((PER, PER), (CLO, OPN))), ((33, 9), ((OPN, CLO), (OPN, OPN))), ((5, 4, 9), ((OPN, CLO), (PER, PER), (CLO, CLO))),
                     ((1, 2, 3), ((PER, PER), (CLO, OPN), (OPN, OPN))), ((3, 5, 70), ((CLO, CLO), (OPN, CLO), (PER, PER)))]


def run_grid_sample(ctx, mem, shape, codes, dtype, shared_values):
    del RECORDS[:]
    try:
        check_grid_sample(ctx, mem, shape, codes, dtype, batch=2, points=301, shared_values=shared_values, seed=len(shape))
        check_grid_sample(ctx, mem, shape, codes, dtype, batch=1, points=4099, shared_values=shared_values, seed=7, graded=True)     # more than one workgroup, ragged
    finally:
        report()


# ---- tightness canary (measured on the reference, not on the code under test) -----------------------------------------------------------------------------------
def oracle32_worst_ratio(res, bc, dt=0.7, kind="random", seed=0, batch=2):
    """ the fp32 oracle (absolute coordinates in fp32) against the bound of the fp32 kernels: worst error / bound per entry point """
    dom, grid, v, f, s, s_codes, s_consts, rng = make_inputs(res, bc, np.float32, batch, dt, kind, seed)
    out = {}
    for entry, exp in (("advect_staggered[self]", expect_advect_staggered(v, v, dt, dom, np.float32)),
                       ("advect_centered", expect_advect_centered(s, v, dt, dom, np.float32, s_codes, s_consts))):
        out[entry] = max(float(e.ratio(e.oracle32).max()) for e in exp)
    return out


# ---- the hand-derived limiter table (tests/limiter_table.py) --------------------------------------------------------------------------------------------------
def check_limiter_table(ctx, mem, dtype):
    """ fwd, bwd, lo, hi and the limited result of the kernels against literals worked out by hand, centred and staggered: equality (the arithmetic is exact) """
    import limiter_table as T
    res, dt = T.RES, T.DT
    row = lambda x: np.asarray(x, dtype).reshape(1, 1, -1)

    def same(got, want, what):
        got = mem.to_host(got)
        assert np.array_equal(got, row(want)), f"limiter table ({np.dtype(dtype).name}), {what}: kernel {got.ravel().tolist()} vs hand-derived {list(want)}"

    try:
        ctx.set_advect_windows_2d(True)
        for halo in (-1, 1, 2, 0):
            ctx.set_advect_halo(halo)
            # centred
            bc = ((PER, PER), (OPN, OPN))
            dom, grid = make_case(res, bc, dtype, 1)
            s_codes, s_consts = ((PER, PER), (CLO, OPN)), [(0.0, 0.0), T.CEN_CONSTS]
            v = [mem.to_dev(np.zeros((1,) + dom.comp_shape(0), dtype)), mem.to_dev(row(T.CEN_FACES))]
            s, fwd, bwd, out, lo, hi = mem.to_dev(row(T.CEN_S)), *(mem.empty((1,) + res, dtype) for _ in range(5))
            ctx.advect_centered(grid, mem.ptr(s), s_codes, s_consts, _P(mem, v), mem.ptr(fwd), dt)
            ctx.advect_centered(grid, mem.ptr(fwd), s_codes, s_consts, _P(mem, v), mem.ptr(bwd), -dt)
            ctx.mac_cormack_centered(grid, mem.ptr(s), s_codes, s_consts, _P(mem, v), mem.ptr(out), dt, 1.0)
            mem.sync()
            same(fwd, T.CEN_FWD, f"centred fwd, halo {halo}"); same(bwd, T.CEN_BWD, f"centred bwd, halo {halo}"); same(out, T.CEN_OUT, f"centred result, halo {halo}")
            # staggered
            bc = ((PER, PER), (CLO, OPN))
            bcv = np.zeros((2, 2, 2))
            bcv[1][0][1] = T.STAG_WALL
            dom, grid = make_case(res, bc, dtype, 1, bc_val=bcv)
            zero = np.zeros((1,) + dom.comp_shape(0), dtype)
            v = [mem.to_dev(zero), mem.to_dev(row(T.STAG_W))]
            g = [mem.to_dev(zero), mem.to_dev(row(T.STAG_G))]
            fwd, bwd, out = ([mem.empty(zero.shape, dtype), mem.empty((1, 1, 8), dtype)] for _ in range(3))
            ctx.advect_staggered(grid, _P(mem, g), _P(mem, v), _P(mem, fwd), dt)
            ctx.advect_staggered(grid, _P(mem, fwd), _P(mem, v), _P(mem, bwd), -dt)
            ctx.mac_cormack_staggered(grid, _P(mem, g), _P(mem, v), _P(mem, out), dt, 1.0)
            mem.sync()
            same(fwd[1], T.STAG_FWD, f"staggered fwd, halo {halo}"); same(bwd[1], T.STAG_BWD, f"staggered bwd, halo {halo}"); same(out[1], T.STAG_OUT, f"staggered result, halo {halo}")
            assert not mem.to_host(out[0]).any(), "limiter table: the zero component along the periodic cell moved"
        # lo / hi: phihip_grid_sample's exact taps at the hand-derived limiter coordinates (centred: the backward points; staggered: the cell frame)
        for vals, coords, lo_w, hi_w, codes, consts in ((T.CEN_S, T.CEN_BACK, T.CEN_LO, T.CEN_HI, ((PER, PER), (CLO, OPN)), T.CEN_CONSTS),
                                                        (T.STAG_G, T.STAG_LIMIT_COORD, T.STAG_LO, T.STAG_HI, ((PER, PER), (CLO, OPN)), (T.STAG_WALL, 0.0))):
            bc_val = [[[0.0, 0.0, 0.0]] * 2, [[consts[0], 0.0, 0.0], [consts[1], 0.0, 0.0]]]
            grid = C.make_grid(2, C.PHIHIP_F64 if np.dtype(dtype) == np.float64 else C.PHIHIP_F32, 1, res, (0.0, 0.0), (1.0, 1.0), codes, bc_val)
            dvals, dc = mem.to_dev(row(vals)), [mem.to_dev(np.zeros((1, 8), dtype)), mem.to_dev(np.asarray(coords, dtype).reshape(1, 8))]
            o, lo, hi = (mem.empty((1, 8), dtype) for _ in range(3))
            ctx.grid_sample(grid, mem.ptr(dvals), 1, _P(mem, dc), 8, mem.ptr(o), mem.ptr(lo), mem.ptr(hi))
            mem.sync()
            assert np.array_equal(mem.to_host(lo).ravel(), np.asarray(lo_w, dtype)) and np.array_equal(mem.to_host(hi).ravel(), np.asarray(hi_w, dtype)), \
                f"limiter table: window {mem.to_host(lo).ravel().tolist()} .. {mem.to_host(hi).ravel().tolist()} vs hand-derived {lo_w} .. {hi_w}"
    finally:
        ctx.set_advect_halo(-1)
        ctx.set_advect_windows_2d(False)


# ---- case tables -----------------------------------------------------------------------------------------------------------------------------------------------
# tiles: T1 = 8 (fp32) / 16 (fp64) rows, T2 = 64 lanes (fp32) / 32 (fp64) along the fast axis, reach 1 or 2: extents one below, at and above a tile on both
# tiled axes next to inside tiles; rows that are no whole 16-byte vectors; LDS-DMA windows with partial tiles on both axes; (res, bc, batch)
CASES = [
    ((16, 20), ((CLO, CLO), (CLO, CLO)), 2), ((16, 20), ((OPN, OPN), (CLO, OPN)), 2), ((7, 13), ((CLO, OPN), (PER, PER)), 1), ((10, 18), ((PER, PER), (OPN, CLO)), 2),
    ((9, 7, 10), ((CLO, CLO), (OPN, OPN), (CLO, OPN)), 2), ((6, 20, 72), ((CLO, OPN), (PER, PER), (CLO, CLO)), 1), ((12, 16, 72), ((PER, PER), (PER, PER), (OPN, OPN)), 2),
    ((12, 16, 70), ((PER, PER), (OPN, OPN), (PER, PER)), 1), ((5, 6, 134), ((PER, PER), (CLO, OPN), (CLO, CLO)), 2), ((4, 5, 24), ((OPN, CLO), (CLO, CLO), (PER, PER)), 2),
    ((17, 30, 131), ((CLO, OPN), (OPN, CLO), (CLO, CLO)), 1), ((21, 30, 136), ((OPN, OPN), (PER, PER), (PER, PER)), 1),
]
CANARY_CASE = CASES[8]
# MI355X only, one dt each: (res, bc, batch, dt)
DEVICE_CASES = [((24, 40, 128), ((PER, PER),) * 3, 1, 0.7), ((40, 36, 256), ((CLO, CLO),) * 3, 1, 2.9), ((24, 44, 200), ((OPN, CLO), (PER, PER), (CLO, OPN)), 1, 0.7),
                ((3, 5, 264), ((PER, PER), (OPN, OPN), (OPN, CLO)), 2, 2.9)]


def case_id(case):
    return "x".join(str(n) for n in case[0]) + "-" + "".join("pco"[lo] + "pco"[hi] for lo, hi in case[1])

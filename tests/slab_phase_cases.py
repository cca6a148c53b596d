"""
Element-wise parity of the slab-decomposed CG phases -- phihip_slab_residual / _matvec / _update / _state (phiflow_amd/csrc/cg.hip), i.e. MODE_RESID, MODE_MATVEC and
MODE_UPDATE of stencil_march.hpp with NB_HALO planes -- in fp32 and fp64, through the C ABI. Used by tests/test_slab_phases_emu.py (emulation),
tests/test_gpu_slab_phases.py (MI355X) and tests/fuzz_parity.py. DESIGN.md "f15" holds the derivation of the constants below.

Ranks are emulated in one process: one Context per rank (the control block and slab_cur live in the context), the "exchange" is a host-side slice of the global array
(plane (b0 - 1) % n0 below, plane b1 % n0 above), the "all-reduce" a float64 sum of the ranks' sums in rank order. Cell flags come from project_ref.cell_flags on the
GLOBAL accessibility mask and are sliced, so the bits of the cells at a cut describe the real neighbour.

Reference: float64 NumPy on the UNDIVIDED grid (project_ref.masked_laplace, pinned <= 1e-12 S to oracle.masked_laplace on every evaluation), on the inputs after
rounding to the element type -- in a chain: on the kernels' own previous outputs. Rule per element, no sample dropped or masked:
        |kernel - ref| <= (K eps + K_REF eps64) M
    M   the phase's expression on magnitudes: |rhs| + S(x);  |r| + |beta| |d_old|;  |x| + |alpha| |d|;  |r| + |alpha| S(d)   (S: the stencil on |source| with |weights|)
    K   counted from the kernel source, one u = eps / 2 per rounding, rounded up to whole eps
The sums are compared with the float64 sum of the reference's elements: the elements' bounds carried through the product, plus the accumulation (a row's V products in
the element type, everything else in double). Output buffers start as NaN bytes, in-place buffers from their input; a frozen batch entry keeps its bits.
"""
import numpy as np

import project_ref as R
from parity_cases import CLO, OPN, PER, C, O
from project_elementwise_cases import (EPS64, K_LAP_FLAGS, K_LAP_FLUX, K_REF, KINDS, RECORDS, TILE_SHAPES, _bits, _cdiv, available_tiles, compare, empty, eps_of,
                                       make_inputs, march_vector_width, pin, report, to_dev)

FAM_RESID, FAM_MATVEC, FAM_UPDATE = 0, 1, 2          # set_tuning_kernel / query_plan: the residual runs the APPLY family's plan
# rounding counts on top of A's (K_LAP_FLUX[3] = 3: 6 u, K_LAP_FLAGS[3] = 4: 8 u of S), u = eps / 2 each, K = count / 2 rounded up to whole eps
K_RESID = 1.0        # stencil_march.hpp:877 r = y - q: 1 u of |y| + |q|                                                          -> 2 K_A + 1 u of |rhs| + S(x)
K_DIR = 1.0          # :548 fma(beta, d_old, r): ONE rounding (the reference takes beta rounded to T already, as :537 does)          -> 1 u of |r| + |beta| |d_old|
K_X = 1.0            # :897 x + alpha * d: the product and the sum, 2 u (contracted, RAG's and cg_axpy_x's explicit fma: 1 u)            -> 2 u of |x| + |alpha| |d|
K_R = 1.0            # :898 r - alpha * q: the product and the difference, 2 u on top of q's 2 K_A u                              -> 2 K_A + 2 u of |r| + |alpha| S(d)
SLAB_BCS = [(PER, PER), (CLO, OPN), (OPN, CLO)]


def k_a(flags):
    return K_LAP_FLAGS[3] if flags else K_LAP_FLUX[3]


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


# ---- the control block, restated (stencil_march.hpp:107-160 cg_advance: PRO_FIRST, PRO_BETA, PRO_ALPHA) --------------------------------------------------------------
def _cg_finite(v):
    return v == v and -1.7e308 <= v <= 1.7e308


def advance(kind, s, sum1, sum2, solve):
    s = dict(s)
    if kind == "first":
        t1, t2 = solve.rel_tol * solve.rel_tol * sum2, solve.abs_tol * solve.abs_tol
        s.update(alpha=0.0, beta=0.0, dq=0.0, rsq=sum1, rsq0=sum1, rhs_sq=sum2, tol_sq=t1 if t1 > t2 else t2, iterations=0)
        s["diverged"] = 0 if _cg_finite(sum1) else 1
        s["converged"] = 1 if sum1 <= s["tol_sq"] else 0
        s["cont"] = int(not s["converged"] and not s["diverged"] and solve.max_iterations > 0)
    elif kind == "beta" and s["cont"]:
        s["beta"] = sum1 / s["rsq"] if s["rsq"] != 0 else 0.0
        s["rsq"] = sum1
        s["diverged"] = int(not _cg_finite(sum1) or (s["rsq0"] > 0 and sum1 / s["rsq0"] > 100 and s["iterations"] >= 8))
        s["converged"] = 1 if sum1 <= s["tol_sq"] else 0
        s["cont"] = int(not s["converged"] and not s["diverged"] and s["iterations"] < solve.max_iterations)
    elif kind == "alpha" and s["cont"]:
        s["iterations"] += 1
        s["dq"] = sum1
        s["alpha"] = s["rsq"] / sum1 if sum1 != 0 else 0.0
    return s


# ---- one problem split over emulated ranks -----------------------------------------------------------------------------------------------------------------------
def slab_masks(res, cuts, rng):
    """ accessible / active 0-1 masks [*res]: a column ACROSS the first cut (rows 0, columns 0-1: the cut's faces closed between two inaccessible cells), a block
    that ENDS at it (plane c - 1, row 1, columns 2-3: a closed face below accessible, active cells of the next rank) and one that STARTS at the last cut (row n1 - 1,
    columns 1-2); active: 90 % at random, so identity rows occur """
    n0, n1, n2 = res
    acc = np.ones(res, np.uint8)
    c, c2 = cuts[1], cuts[-2] % n0
    acc[c - 1:c + 1, 0, 0:2] = 0
    acc[c - 1, 1, 2:4] = 0
    acc[c2, n1 - 1, 1:3] = 0
    act = (rng.random(res) < 0.9).astype(np.uint8)
    act[c % n0, 1, 2:4] = 1
    act[c2, 0, n2 - 2] = 1
    return acc, act


class World:
    """ one global problem [batch, *res] cut along axis 0 at `cuts`; fields live as one device buffer per rank, `host` holds their global host copies """
    def __init__(self, ctxs, mem, res, bc, dtype, cuts, kind="random", flags=False, seed=0, batch=2, offset=0, tamper=None, force=None):
        i1 = make_inputs(res, bc, dtype, batch, "random" if kind == "nonfinite" else kind, seed)
        i2 = make_inputs(res, bc, dtype, batch, "random" if kind == "nonfinite" else kind, seed + 1)
        self.mem, self.res, self.bc, self.dtype, self.batch, self.kind, self.offset, self.tamper = mem, tuple(res), bc, dtype, batch, kind, offset, tamper
        self.dom, self.dx, self.rng, self.eps = i1.dom, i1.dom.dx, i1.rng, eps_of(dtype)
        self.cuts, self.nr, self.n0 = list(cuts), len(cuts) - 1, res[0]
        assert cuts[0] == 0 and cuts[-1] == res[0] and all(a < b for a, b in zip(cuts, cuts[1:])) and self.nr <= len(ctxs)
        self.ctxs = list(ctxs[:self.nr])
        periodic = bc[0][0] == PER
        self.halo = [(k > 0 or periodic, k < self.nr - 1 or periodic) for k in range(self.nr)]
        code = C.PHIHIP_F64 if np.dtype(dtype) == np.float64 else C.PHIHIP_F32
        lo, up, h0 = self.dom.lower, self.dom.upper, self.dx[0]
        self.grids = [C.make_grid(3, code, batch, (b1 - b0,) + self.res[1:], (lo[0] + b0 * h0,) + tuple(lo[1:]), (lo[0] + b1 * h0,) + tuple(up[1:]), bc, self.dom.bc_val)
                      for b0, b1 in zip(cuts, cuts[1:])]
        self.flags = self.acc = self.active = self.hard = None
        self.dflags = [None] * self.nr
        if flags:
            acc, act = slab_masks(self.res, self.cuts, self.rng)
            self.flags = R.cell_flags(acc, act, self.res, bc, False)
            self.acc, self.active = acc[None], ((self.flags >> 6) & 1)[None]
            self.hard = [R.accessible_faces(self.acc, d, self.res, bc).astype(np.float64) for d in range(3)]
            for k, (b0, b1) in enumerate(zip(cuts, cuts[1:])):
                # the negative control: flags from the slab's OWN box, the cut faces under the local boundary rule
                f = R.cell_flags(acc[b0:b1], act[b0:b1], (b1 - b0,) + self.res[1:], bc, False) if tamper == "localflags" else self.flags[b0:b1]
                self.dflags[k] = to_dev(mem, f, offset)
        self.host, self.dev = {}, {}
        for name, a in (("x", i1.p), ("rhs", i1.s), ("r2", i2.p), ("d0", i2.s)):
            self.put(name, a)
        self.state = [dict(cont=0, iterations=0, converged=0, diverged=0, rsq=0.0, rhs_sq=0.0, alpha=0.0, beta=0.0) for _ in range(batch)]
        self.solve = C.Solve(1e-30, 0.0, 100, 0, 0, 0)
        self.count = None          # negative controls: a number -> violations are counted, not raised
        self.trace = []            # bits of every array read back, in order
        self.keep = []             # device buffers of the launch in flight
        vec = march_vector_width(res[-1], dtype, bool(offset))
        self.path = f"vec={vec} flags={'yes' if flags else 'no'} a0={'pco'[bc[0][0]]}{'pco'[bc[0][1]]} cuts={','.join(map(str, cuts))}{' unaligned' if offset else ''}"
        self.forced = False
        if force is not None:
            self.force(*force)

    # -- memory
    def slabs(self, a):
        return [a[:, b0:b1] for b0, b1 in zip(self.cuts, self.cuts[1:])]

    def put(self, name, a):
        self.host[name] = np.ascontiguousarray(a)
        self.dev[name] = [to_dev(self.mem, s, self.offset) for s in self.slabs(a)]

    def new(self, name):
        self.host[name] = np.full((self.batch,) + self.res, np.nan, self.dtype)
        self.dev[name] = [empty(self.mem, s.shape, self.dtype, self.offset) for s in self.slabs(self.host[name])]

    def pull(self, name):
        self.mem.sync()
        self.host[name] = np.concatenate([self.mem.to_host(h) for h in self.dev[name]], axis=1)
        self.trace.append(_bits(self.host[name]).copy())
        return self.host[name]

    def ptr(self, name, k):
        return self.mem.ptr(self.dev[name][k])

    def fl(self, k):
        return self.mem.ptr(self.dflags[k]) if self.dflags[k] is not None else 0

    def scalars(self, values):
        h = self.mem.to_dev(np.asarray(values, np.float64))
        self.keep.append(h)
        return self.mem.ptr(h)

    def planes(self, G, k):
        """ the exchange: (lower, upper) halo pointers of rank k from the global array G, with the negative controls' wrong inputs """
        b0, b1 = self.cuts[k], self.cuts[k + 1]
        lo = G[:, (b0 - 1) % self.n0].copy() if self.halo[k][0] else None
        hi = G[:, b1 % self.n0].copy() if self.halo[k][1] else None
        if self.tamper == "swap" and lo is not None and hi is not None:
            lo, hi = hi, lo
        elif self.tamper == "entry":
            for h in (lo, hi):
                if h is not None:
                    h[1] = h[0]
        elif self.tamper == "zero":
            (lo if lo is not None else hi)[...] = 0
        hs = [None if h is None else to_dev(self.mem, h, self.offset) for h in (lo, hi)]
        self.keep += hs
        return tuple(0 if h is None else self.mem.ptr(h) for h in hs)

    # -- plans
    def plan(self, k, fam):
        return self.ctxs[k].query_plan(self.grids[k], self.flags is not None, fam)

    def force(self, tid, chunk):
        """ tile `tid` and `chunk` planes for the three families on every rank, asserted with query_plan; `release()` restores """
        rows, tpr = TILE_SHAPES[tid]
        vec = march_vector_width(self.res[-1], self.dtype)
        one = vec == 1 or vec < 0
        self.forced = True
        for k, ctx in enumerate(self.ctxs):
            for fam in (FAM_RESID, FAM_MATVEC, FAM_UPDATE):
                ctx.set_tuning_kernel(fam, rows, tpr, chunk)
                plan = self.plan(k, fam)
                want = dict(rows=1 if one else rows, tpr=64 if one else tpr, vec=vec, chunk=min(chunk, self.cuts[k + 1] - self.cuts[k]))
                assert {n: plan[n] for n in want} == want, f"rank {k} family {fam} {self.res} {np.dtype(self.dtype).name}: plan {plan}, expected {want}"
        self.path += f" tile={tid} chunk={chunk}"

    def release(self):
        if self.forced:
            for ctx in self.ctxs:
                for fam in (FAM_RESID, FAM_MATVEC, FAM_UPDATE):
                    ctx.set_tuning_kernel(fam, 0, 0, 0)

    # -- reference
    def A(self, p64, what):
        """ (A p, S) in float64 on the undivided grid, pinned to the oracle; S from the finite part of p, so that it is finite wherever A p is """
        with np.errstate(invalid='ignore', over='ignore'):
            val = R.masked_laplace(p64, self.res, self.bc, self.dx, self.acc, self.active)[0]
            S = self.S(_fin(p64))
            pin(val, O.masked_laplace(p64, self.dom, self.hard, None if self.active is None else self.active.astype(np.float64)), S, f"masked_laplace ({what})")
        return val, S

    def S(self, mag):
        return R.masked_laplace(mag, self.res, self.bc, self.dx, self.acc, self.active)[1]

    def running(self):
        return np.asarray([bool(s["cont"]) for s in self.state])

    # -- comparison
    def cmp(self, entry, got, ref, bound):
        if self.count is None:
            return compare(entry, self.path, self, self.kind, got, ref, bound)
        g = got.astype(np.float64)
        fin = np.isfinite(ref)
        with np.errstate(invalid='ignore'):
            bad = (np.isnan(g) != np.isnan(ref)) | (np.isinf(g) != np.isinf(ref)) | (fin & np.isfinite(g) & (np.abs(g - ref) > bound))
        self.count += int(bad.sum())

    def same_bits(self, what, now, before, entries):
        for b in entries:
            assert np.array_equal(_bits(now[b]), _bits(before[b])), f"{what} [{self.path}]: entry {b} is frozen and changed"

    def sums(self, entry, fam, got, a, b, Ba, Bb, run):
        """ per rank and running entry: got[k][e] against sum a b over the rank's own cells. Bound: sum |a| Bb + |b| Ba + Ba Bb (the elements' bounds carried through
        the product) + (V u + (n64 u64 + K_REF eps64)) sum (|a| + Ba)(|b| + Bb): a row's V products are added up in T (V roundings on the first term), the rest
        in double -- n64 = chunk x rows per thread + the two 6 + 4 trees + ceil(nblk / 256) additions of sum_partials_kernel """
        for k, (sa, sb, sBa, sBb) in enumerate(zip(self.slabs(a), self.slabs(b), self.slabs(Ba), self.slabs(Bb))):
            plan = self.plan(k, fam)
            n64 = plan["chunk"] * plan["rows"] + _cdiv(plan["nblk"], 256) + 20
            with np.errstate(invalid='ignore', over='ignore'):
                ref = (sa * sb).sum(axis=(1, 2, 3))
            fa, fb = np.abs(_fin(sa)), np.abs(_fin(sb))
            bound = (fa * sBb + fb * sBa + sBa * sBb).sum(axis=(1, 2, 3)) \
                + (0.5 * abs(plan["vec"]) * self.eps + (0.5 * n64 + K_REF) * EPS64) * ((fa + sBa) * (fb + sBb)).sum(axis=(1, 2, 3))
            self.cmp(entry, np.asarray(got[k], np.float64)[run], ref[run], bound[run])


def allreduce(per_rank):
    total = np.zeros_like(per_rank[0])
    for s in per_rank:
        total = total + s
    return total


# ---- the phases ----------------------------------------------------------------------------------------------------------------------------------------------------
def residual(w, keep_going=False):
    """ r = rhs - A x; sums = [sum r^2, sum rhs^2] per entry over the rank's own cells. keep_going: frozen entries are skipped (their r keeps its bits; their sums
    are unspecified: the kernel returns before it writes its partials). Returns the ranks' sums """
    X, Y = w.host["x"], w.host["rhs"]
    run = w.running() if keep_going else np.ones(w.batch, bool)
    Ax, Sx = w.A(X.astype(np.float64), "residual")
    with np.errstate(invalid='ignore'):
        ref = Y.astype(np.float64) - Ax
    bound = ((k_a(w.flags is not None) + K_RESID) * w.eps + K_REF * EPS64) * (np.abs(_fin(Y.astype(np.float64))) + Sx)
    if "r" not in w.dev:
        w.new("r")
    before = w.host["r"]
    out = []
    for k, ctx in enumerate(w.ctxs):
        ds = empty(w.mem, (2 * w.batch,), np.float64)
        ctx.slab_residual(w.grids[k], w.halo[k], w.fl(k), w.ptr("x", k), w.planes(X, k), w.ptr("rhs", k), w.ptr("r", k), w.mem.ptr(ds), keep_going)
        w.mem.sync()
        out.append(w.mem.to_host(ds).astype(np.float64))
    del w.keep[:]
    got = w.pull("r")
    w.cmp("slab_residual", got[run], ref[run], bound[run])
    w.same_bits("slab_residual", got, before, np.flatnonzero(~run))
    w.sums("slab_residual sum r^2", FAM_RESID, [s[:w.batch] for s in out], ref, ref, bound, bound, run)
    zero = np.zeros_like(bound)
    # (and against the sum of the kernel's OWN elements: nothing carried, the accumulation alone -- the row that sees a plane counted twice or not at all)
    w.sums("slab_residual sum r^2 | own", FAM_RESID, [s[:w.batch] for s in out], got.astype(np.float64), got.astype(np.float64), zero, zero, run)
    w.sums("slab_residual sum rhs^2", FAM_RESID, [s[w.batch:] for s in out], Y.astype(np.float64), Y.astype(np.float64), zero, zero, run)
    w.trace += [s[np.concatenate([run, run])].copy().view(np.uint64) for s in out]
    return out


def matvec(w, first, sums_in, r="r", d_old="d0", d_new="d1"):
    """ d_new = fma(beta, d_old, r) with beta rounded to the element type (first: beta = 0, d_new = r exactly); sum_out = sum d_new (A d_new) over the own cells, the
    neighbours' planes of d_new rebuilt from the r and d halos by the same fma """
    T = w.dtype
    Rg, Dg = w.host[r], w.host[d_old]
    w.state = [advance("first" if first else "beta", s, float(sums_in[b]), float(sums_in[w.batch + b]), w.solve) for b, s in enumerate(w.state)]
    run = w.running()
    beta = np.asarray([float(T(s["beta"])) for s in w.state]).reshape(-1, 1, 1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        ref = Rg.astype(np.float64) if first else beta * Dg.astype(np.float64) + Rg.astype(np.float64)
    Bd = np.zeros(ref.shape) if first else (K_DIR * w.eps + K_REF * EPS64) * (np.abs(_fin(Rg.astype(np.float64))) + np.abs(beta) * np.abs(_fin(Dg.astype(np.float64))))
    q, Sd = w.A(ref, "matvec")
    SB = w.S(Bd)
    Bq = (k_a(w.flags is not None) * w.eps + K_REF * EPS64) * (Sd + SB) + SB
    if d_new not in w.dev:
        w.new(d_new)
    before = w.host[d_new]
    dsum_in = w.scalars(sums_in)
    out = []
    for k, ctx in enumerate(w.ctxs):
        ds = empty(w.mem, (w.batch,), np.float64)
        ctx.slab_matvec(w.grids[k], w.halo[k], w.fl(k), first, dsum_in, w.ptr(r, k), w.planes(Rg, k), w.ptr(d_old, k), w.planes(Dg, k), w.ptr(d_new, k), w.mem.ptr(ds), w.solve)
        w.mem.sync()
        out.append(w.mem.to_host(ds).astype(np.float64))
    del w.keep[:]
    got = w.pull(d_new)
    name = "slab_matvec first" if first else "slab_matvec"
    w.cmp(name, got[run], ref[run], Bd[run])
    w.same_bits(name, got, before, np.flatnonzero(~run))
    w.sums(name + " sum d Ad", FAM_MATVEC, out, ref, q, Bd, Bq, run)
    # (and on the kernel's OWN d_new, whose planes across a cut are the neighbour's own output bit for bit: only A's bound is carried)
    q_own, S_own = w.A(got.astype(np.float64), "matvec, own d_new")
    w.sums(name + " sum d Ad | own", FAM_MATVEC, out, got.astype(np.float64), q_own, np.zeros_like(Bd), (k_a(w.flags is not None) * w.eps + K_REF * EPS64) * S_own, run)
    w.trace += [s[run].copy().view(np.uint64) for s in out]
    return out


def update(w, sum_in, d="d1", x_only=False):
    """ alpha = rsq / sum_in, rounded to the element type; x += alpha d; r -= alpha (A d); sum_out = sum r_new^2. x_only (the refresh): only x changes """
    T = w.dtype
    Dg, X, Rg = w.host[d], w.host["x"], w.host["r"]
    w.state = [advance("alpha", s, float(sum_in[b]), 0.0, w.solve) for b, s in enumerate(w.state)]
    run = w.running()
    frozen = np.flatnonzero(~run)
    alpha = np.asarray([float(T(s["alpha"])) for s in w.state]).reshape(-1, 1, 1, 1)
    D64 = Dg.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        ref_x = X.astype(np.float64) + alpha * D64
    Bx = (K_X * w.eps + K_REF * EPS64) * (np.abs(_fin(X.astype(np.float64))) + np.abs(alpha) * np.abs(_fin(D64)))
    if not x_only:
        q, Sd = w.A(D64, "update")
        with np.errstate(invalid='ignore', over='ignore'):
            ref_r = Rg.astype(np.float64) - alpha * q
        Br = ((k_a(w.flags is not None) + K_R) * w.eps + K_REF * EPS64) * (np.abs(_fin(Rg.astype(np.float64))) + np.abs(alpha) * Sd)
    dsum_in = w.scalars(sum_in)
    out = []
    for k, ctx in enumerate(w.ctxs):
        ds = empty(w.mem, (w.batch,), np.float64)
        ctx.slab_update(w.grids[k], w.halo[k], w.fl(k), dsum_in, w.ptr(d, k), (0, 0) if x_only else w.planes(Dg, k), w.ptr("x", k), 0 if x_only else w.ptr("r", k),
                        0 if x_only else w.mem.ptr(ds), w.solve, x_only)
        w.mem.sync()
        out.append(w.mem.to_host(ds).astype(np.float64))
    del w.keep[:]
    got_x, got_r = w.pull("x"), w.pull("r")
    name = "slab_update x_only" if x_only else "slab_update"
    w.cmp(name + " x", got_x[run], ref_x[run], Bx[run])
    w.same_bits(name + " x", got_x, X, frozen)
    if x_only:
        w.same_bits(name + " r", got_r, Rg, range(w.batch))
        return None
    w.cmp(name + " r", got_r[run], ref_r[run], Br[run])
    w.same_bits(name + " r", got_r, Rg, frozen)
    w.sums(name + " sum r^2", FAM_UPDATE, out, ref_r, ref_r, Br, Br, run)
    w.sums(name + " sum r^2 | own", FAM_UPDATE, out, got_r.astype(np.float64), got_r.astype(np.float64), np.zeros_like(Br), np.zeros_like(Br), run)
    w.trace += [s[run].copy().view(np.uint64) for s in out]
    return out


def state(w, first, sums_in, peek=False):
    """ phihip_slab_state against cg_advance(PRO_FIRST | PRO_BETA) restated: every field of SolveInfo, on every rank; peek: the chain does not advance """
    model = [advance("first" if first else "beta", s, float(sums_in[b]), float(sums_in[w.batch + b]), w.solve) for b, s in enumerate(w.state)]
    dsum_in = w.scalars(sums_in)
    for k, ctx in enumerate(w.ctxs):
        infos = ctx.slab_state(w.grids[k], first, dsum_in, w.solve, peek)
        for b, (i, m) in enumerate(zip(infos, model)):
            got = (i.iterations, i.converged, i.diverged, i.residual_sq, i.rhs_sq, i.reserved)
            want = (m["iterations"], m["converged"], m["diverged"], m["rsq"], m["rhs_sq"], m["cont"])
            if w.count is None:
                assert got == want, f"slab_state(first={first}, peek={peek}) [{w.path}] rank {k} entry {b}: (iterations, converged, diverged, residual_sq, rhs_sq, reserved) {got}, expected {want}"
    del w.keep[:]
    if not peek:
        w.state = model
    RECORDS.append(dict(entry="slab_state peek" if peek else "slab_state", path=w.path, dtype=np.dtype(w.dtype).name, res="x".join(map(str, w.res)), kind=w.kind, ratio=0.0))
    return model


# ---- single phases with scalars the caller chooses -------------------------------------------------------------------------------------------------------------------
def plant_nonfinite(w, name):
    """ NaN into one halo plane (the last plane below the first cut; with flags: an inaccessible cell whose upper neighbour is accessible and active -- the kernel's
    `if (f & bit)` must keep it out) and into one own cell (the first plane above the last cut, accessible and active), both in entry 0 """
    a = w.host[name].copy()
    a[0, w.cuts[1] - 1, 1, 2] = np.nan
    a[0, w.cuts[-2] % w.n0, 0, w.res[2] - 2] = np.nan
    w.put(name, a)


def phases(w):
    """ residual; the control block from chosen sums; MATVEC with beta = 1/2 and 2/5 on an independent r; UPDATE with alpha < 0 and > 0 on that d_new; the x-only step """
    if w.kind == "nonfinite":
        plant_nonfinite(w, "x")
        plant_nonfinite(w, "r2")
    assert w.batch == 2
    residual(w)
    state(w, True, [2.0, 3.0, 5.0, 7.0])
    matvec(w, False, [1.0, 1.2, 0.0, 0.0], r="r2", d_old="d0", d_new="d1")
    update(w, [-3.0, 2.5], d="d1")
    matvec(w, False, [0.7, 0.9, 0.0, 0.0], r="r", d_old="d1", d_new="d0")
    update(w, [4.0, -5.0], d="d1", x_only=True)
    state(w, False, [0.5, 0.25, 0.0, 0.0])


def run_phases(ctxs, mem, res, bc, dtype, cuts, kinds=("random",), flags=(False, True), seed=0, offset=0, force=None):
    del RECORDS[:]
    try:
        for kind in kinds:
            for fl in flags:
                w = World(ctxs, mem, res, bc, dtype, cuts, kind, fl, seed, offset=offset, force=force)
                try:
                    phases(w)
                finally:
                    w.release()
    finally:
        report()


# ---- the one-step chain --------------------------------------------------------------------------------------------------------------------------------------------
def chain(ctxs, mem, res, bc, dtype, cuts, flags=True, seed=0, peeks=True, max_iterations=3, force=None):
    """ residual, matvec(first), update, matvec, update, matvec, update(x_only), residual(keep_going), matvec, slab_state: every phase against the reference applied to
    the kernels' own previous outputs, every rank fed the float64 sum over the ranks of the kernels' own sums. Entry 1 is converged at the start: rhs = A x + 1e-3 noise,
    abs_tol between the two entries' initial residuals (decided by the reference alone). Returns the trace of bits """
    w = World(ctxs, mem, res, bc, dtype, cuts, "random", flags, seed, force=force)
    try:
        X = w.host["x"].astype(np.float64)
        rhs = w.host["rhs"].copy()
        rhs[1] = (w.A(X, "setup")[0][1] + 1e-3 * rhs[1]).astype(dtype)
        w.put("rhs", rhs)
        rr = ((rhs.astype(np.float64) - w.A(X, "setup")[0]) ** 2).sum(axis=(1, 2, 3))
        assert rr[1] < 1e-4 * rr[0]
        w.solve = C.Solve(1e-30, float((rr[0] * rr[1]) ** 0.25), max_iterations, 3, 0, 0)
        w.new("d1")
        B = w.batch

        def peek(s):
            if peeks:
                state(w, False, s, peek=True)

        def frozen_entry():
            assert (w.state[1]["cont"], w.state[1]["converged"], w.state[1]["iterations"]) == (0, 1, 0)
        s2 = allreduce(residual(w))                                              # 1
        dq = allreduce(matvec(w, True, s2, "r", "d0", "d1"))                     # 2
        frozen_entry()
        assert w.state[0]["cont"] == 1
        s2 = np.concatenate([allreduce(update(w, dq, "d1")), s2[B:]])            # 3   (entry 1: unspecified sums, never read: its control block is frozen)
        peek(s2)
        dq = allreduce(matvec(w, False, s2, "r", "d1", "d0"))                    # 4
        s2 = np.concatenate([allreduce(update(w, dq, "d0")), s2[B:]])            # 5
        peek(s2)
        dq = allreduce(matvec(w, False, s2, "r", "d0", "d1"))                    # 6
        update(w, dq, "d1", x_only=True)                                         # 7
        peek(s2)
        s2 = allreduce(residual(w, keep_going=True))                             # 8
        peek(s2)
        matvec(w, False, s2, "r", "d1", "d0")                                    # 9   (max_iterations = 3: the entry stops here, d_new keeps its bits)
        final = state(w, False, s2)                                              # 10
        frozen_entry()
        assert final[0]["iterations"] == 3 and final[0]["cont"] == (1 if max_iterations > 3 else 0)
        return [t for t in w.trace]
    finally:
        w.release()


def run_chain(ctxs, mem, res, bc, dtype, cuts, flags=True, seed=0, max_iterations=3, force=None):
    """ the chain with the peeks and without them: identical bits in every array and every running entry's sums """
    del RECORDS[:]
    try:
        a = chain(ctxs, mem, res, bc, dtype, cuts, flags, seed, True, max_iterations, force)
        b = chain(ctxs, mem, res, bc, dtype, cuts, flags, seed, False, max_iterations, force)
        assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b)), "slab_state(peek=1) changed what the chain computes"
    finally:
        report()


# ---- negative controls ---------------------------------------------------------------------------------------------------------------------------------------------
TAMPERS = ("swap", "entry", "zero", "localflags")
CONTROL_CASE = ((7, 5, 12), ((CLO, OPN), (PER, PER), (OPN, CLO)), [0, 2, 5, 7])


def control_counts(ctxs, mem, dtype, seed=0):
    """ the phases with the right inputs (0 violations) and with each wrong one: violations counted by the same checker """
    res, bc, cuts = CONTROL_CASE
    counts = {}
    for tamper in (None,) + TAMPERS:
        w = World(ctxs, mem, res, bc, dtype, cuts, "random", True, seed, tamper=tamper)
        w.count = 0
        phases(w)
        counts[tamper] = w.count
    return counts


def control_separation(dtype, tamper, seed=0):
    """ NumPy only: by how many bounds the residual's REFERENCE moves when the wrong input replaces the right one -- the largest |change of A x| / bound over the
    planes at the cuts """
    res, bc, cuts = CONTROL_CASE

    class NoMem:
        to_dev = staticmethod(lambda a: a)
        ptr = staticmethod(lambda h: 0)
    w = World([None] * 3, NoMem(), res, bc, dtype, cuts, "random", True, seed)
    X = w.host["x"].astype(np.float64)
    Ax, Sx = w.A(X, "control")
    bound = ((k_a(True) + K_RESID) * w.eps + K_REF * EPS64) * (np.abs(w.host["rhs"].astype(np.float64)) + Sx)
    w0 = 1.0 / (w.dx[0] * w.dx[0])
    worst = 0.0
    for k, (b0, b1) in enumerate(zip(cuts, cuts[1:])):
        local = R.cell_flags(w.acc[0][b0:b1], ((w.flags >> 6) & 1)[b0:b1], (b1 - b0,) + tuple(res[1:]), bc, False)
        right = [X[:, (b0 - 1) % w.n0] if w.halo[k][0] else None, X[:, b1 % w.n0] if w.halo[k][1] else None]
        wrong = [None if h is None else h.copy() for h in right]
        if tamper == "swap" and right[0] is not None and right[1] is not None:
            wrong = [right[1], right[0]]
        elif tamper == "entry":
            for h in wrong:
                if h is not None:
                    h[1] = h[0]
        elif tamper == "zero":
            (wrong[0] if wrong[0] is not None else wrong[1])[...] = 0
        for side, plane in ((0, b0), (1, b1 - 1)):
            if right[side] is None:
                continue
            live = ((w.flags[plane] >> side) & 1) * ((w.flags[plane] >> 6) & 1)          # the face is open and the cell's row is the stencil
            if tamper == "localflags":
                change = live * (1 - ((local[plane - b0] >> side) & 1)) * np.abs(right[side] - X[:, plane]) * w0
            else:
                change = live * np.abs(wrong[side] - right[side]) * w0
            worst = max(worst, float((change / bound[:, plane]).max()))
    return worst


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------------------------------
def _bc(k):
    """ the slab axis through SLAB_BCS, the other two through the f12 KINDS """
    return (SLAB_BCS[k % 3], KINDS[k % 5], KINDS[(k + 2) % 5])


def slab_range(n, rank, world):
    base, extra = divmod(n, world)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


UNEVEN7 = [0] + [slab_range(7, r, 3)[1] for r in range(3)]          # [0, 3, 5, 7]
# row widths: (name, dtype name, res, forced (tile, chunk) or None): whole vector, the fp32 two-wide row, ragged >= 2 V, scalar, one row tile
WIDTH_CASES = [("f32", (7, 5, 12), None), ("f32", (7, 5, 10), None), ("f32", (7, 4, 13), None), ("f32", (7, 5, 7), None), ("f32", (5, 3, 264), (8, 64)),
               ("f64", (7, 5, 10), None), ("f64", (7, 4, 13), None), ("f64", (7, 5, 129), None)]
WIDTH_VECS = [4, 2, -4, 1, 4, 2, -2, 1]
# two tiles along each in-plane axis next to the plane halos (tile (1, 16): 16 rows x 16 V columns), and chunks of 1 and 2 planes on a four- and a six-plane slab
TILE_CASES = [("f32", (6, 18, 72), [0, 2, 6], (0, 1)), ("f32", (6, 18, 72), [0, 2, 6], (0, 2)), ("f64", (6, 18, 36), [0, 2, 6], (0, 1)), ("f64", (6, 18, 36), [0, 2, 6], (0, 2)),
              ("f32", (8, 5, 72), [0, 6, 8], (0, 1)), ("f32", (8, 5, 72), [0, 6, 8], (0, 2)), ("f64", (8, 5, 36), [0, 6, 8], (0, 2))]
CHAIN_CASES = [((7, 5, 12), [0, 1, 3, 7], 0), ((7, 4, 13), UNEVEN7, 1), ((6, 5, 10), [0, 2, 6], 2)]
DT = {"f32": np.float32, "f64": np.float64}

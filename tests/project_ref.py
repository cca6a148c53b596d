"""
NumPy restatement of the non-iterative half of fluid.make_incompressible and of the obstacle kernels, written out independently of the library and of oracle/
(tests/project_elementwise_cases.py pins every function to the oracle's float64 result before it is used). Imports nothing under test.

Every function takes an element type: the arithmetic (differences, products, sums, in the order the kernels of phiflow_amd/csrc/project.hip and MODE_APPLY of
stencil_march.hpp use) runs in that type, so the float32 evaluation is the yardstick of the fp32 kernels (the canary, e_ref32). Each returns the value and a
per-sample scale S in float64: the same stencil applied to |inputs| with |weights|, |wall constants| included. S is what a rounding count multiplies.

Reference lines restated (phi = the reference project):
    divergence                phi/field/_field_math.py:617-626 with bake_extrapolation :20-39; `div * active`, is_finite guard phi/physics/fluid.py:139-144
    balance                   fluid._balance_divergence, phi/physics/fluid.py:205-209
    grad_subtract             phi/physics/fluid.py:158-161 (v - hard_bcs * grad p), spatial_gradient at faces phi/field/_field_math.py:535-581,
                              pressure extrapolation phi/physics/fluid.py:264-274
    masked_laplace            fluid.masked_laplace, phi/physics/fluid.py:165-202
    accessible_faces, cell_flags   phi/physics/fluid.py:130-137, _accessible_extrapolation :277-288
    accessible, apply_obstacles    phi/physics/fluid.py:130-133, 212-240; phi/geom/_box.py:127-152,174-185,217-236; phi/geom/_sphere.py; phi/geom/_embed.py:38-66,139-158;
                              phi/geom/_geom_ops.py:96-102,297-319; phi/field/_angular_velocity.py:40-46
    safe_mul                  phiml.math.safe_mul (0 * nan = 0), used by fluid.py:231-239
    centered_to_staggered     sample_grid_at_faces, phi/field/_resample.py:272-276
    diffuse_explicit          phi/physics/diffuse.py:13-60 with field.laplace order 2, phi/field/_field_math.py:119-145

Codes: 0 PERIODIC, 1 CLOSED (velocity: constant wall value; a closed side stores no face), 2 OPEN (zero gradient; the upper face is stored) -- phihip.h PHIHIP_BC_*.
Arrays carry the batch as first axis; spatial axis d is tensor axis d + 1.
"""
import numpy as np

PERIODIC, CLOSED, OPEN = 0, 1, 2
WRAP, EDGE, CONST = "wrap", "edge", "const"


# ---- layout --------------------------------------------------------------------------------------------------------------------------------------------------
def comp_shape(res, bc, d):
    """ stored faces of component d: the lower face of every cell unless the lower side is CLOSED, plus the upper face of the last cell on an OPEN upper side """
    s = list(res)
    s[d] += int(bc[d][0] != CLOSED) + int(bc[d][1] == OPEN) - 1
    return tuple(s)


def face_offset(bc, d):
    """ physical number of stored face 0 """
    return 1 if bc[d][0] == CLOSED else 0


def _sl(nd, ax, i, j):
    return tuple(slice(i, j) if k == ax else slice(None) for k in range(nd))


def _ghost(x, ax, kind_lo, kind_hi, c_lo=0.0, c_hi=0.0):
    """ one ghost layer on each side of tensor axis ax """
    n = x.shape[ax]
    first, last = x[_sl(x.ndim, ax, 0, 1)], x[_sl(x.ndim, ax, n - 1, n)]
    lo = last if kind_lo == WRAP else (first if kind_lo == EDGE else np.full_like(first, c_lo))
    hi = first if kind_hi == WRAP else (last if kind_hi == EDGE else np.full_like(last, c_hi))
    return np.concatenate([lo, x, hi], axis=ax)


def _two(x, ax, n, first):
    """ (lower, upper) neighbours: slices [first, first + n) and [first + 1, first + 1 + n) of the ghosted array """
    return x[_sl(x.ndim, ax, first, first + n)], x[_sl(x.ndim, ax, first + 1, first + 1 + n)]


def _vel_kind(code):
    return WRAP if code == PERIODIC else (CONST if code == CLOSED else EDGE)


def all_faces(vd, d, res, bc, bcv):
    """ the res[d] + 1 faces of component d: the faces a side does not store come from the wall constant bcv[d][side][d] or from the wrap """
    ax = d + 1
    g = _ghost(vd, ax, _vel_kind(bc[d][0]), _vel_kind(bc[d][1]), bcv[d][0][d], bcv[d][1][d])
    first = 0 if bc[d][0] == CLOSED else 1
    return g[_sl(g.ndim, ax, first, first + res[d] + 1)]


# ---- divergence ------------------------------------------------------------------------------------------------------------------------------------------------
def divergence(v, res, bc, bcv, dx, dtype=np.float64):
    """ sum_d (upper face - lower face) * (1 / dx_d), summed from the slowest axis on, starting from 0 (divergence_kernel). Returns (div, S) """
    T = np.dtype(dtype).type
    D = len(res)
    out = S = None
    for d in range(D):
        f = all_faces(np.asarray(v[d], T), d, res, bc, np.asarray(bcv, np.float64).astype(T))
        lo, hi = _two(f, d + 1, res[d], 0)
        r = T(1.0 / dx[d])
        with np.errstate(invalid='ignore', over='ignore'):
            term = (hi - lo) * r
            out = term if out is None else out + term
            s = (np.abs(hi.astype(np.float64)) + np.abs(lo.astype(np.float64))) * abs(1.0 / dx[d])
        S = s if S is None else S + s
    assert out.dtype == T
    return out, S


def mask_divergence(div, active, guard):
    """ div where the cell is active, 0 elsewhere (a selection: non-finite values of inactive cells do not leak); guard: non-finite values -> 0 on every cell.
    With the guard this is the reference's where(is_finite(div * active), div * active, 0). """
    out = div if active is None else np.where(np.broadcast_to(active, div.shape) > 0, div, div.dtype.type(0))
    return np.where(np.isfinite(out), out, div.dtype.type(0)) if guard else out


def balance(div, active, dtype=np.float64):
    """ div - active * sum(div) / sum(active) per batch entry, the sums in float64; an entry without active cells: shift 0, nothing subtracted.
    Returns (balanced, shift [B] float64, active count [B]) """
    T = np.dtype(dtype).type
    B = div.shape[0]
    a = np.ones(div.shape, np.float64) if active is None else np.broadcast_to(np.asarray(active > 0, np.float64), div.shape)
    s = div.astype(np.float64).reshape(B, -1).sum(axis=1)
    n = a.reshape(B, -1).sum(axis=1)
    shift = np.where(n != 0, s / np.where(n != 0, n, 1.0), 0.0)
    sh = shift.astype(T).reshape((B,) + (1,) * (div.ndim - 1))
    out = np.asarray(div, T) - a.astype(T) * sh
    assert out.dtype == T
    return out, shift, n


# ---- pressure gradient ---------------------------------------------------------------------------------------------------------------------------------------
def _pressure_cells(p, d, res, bc):
    """ (p_L, p_R) at the stored faces of component d: wrap on a periodic axis, ghost 0 outside an open side (a closed side stores no face) """
    ax = d + 1
    g = _ghost(p, ax, WRAP if bc[d][0] == PERIODIC else CONST, WRAP if bc[d][1] == PERIODIC else CONST)
    return _two(g, ax, comp_shape(res, bc, d)[d], face_offset(bc, d))


def accessible_faces(acc, d, res, bc):
    """ hard_bcs = stagger(accessible, minimum) at the stored faces of component d; outside the domain: wrap / OPEN 1 / CLOSED 0. acc: 0 / 1 [B or 1, *res] """
    ax = d + 1
    a = (np.asarray(acc) != 0).astype(np.uint8)
    g = _ghost(a, ax, WRAP if bc[d][0] == PERIODIC else CONST, WRAP if bc[d][1] == PERIODIC else CONST, int(bc[d][0] == OPEN), int(bc[d][1] == OPEN))
    lo, hi = _two(g, ax, comp_shape(res, bc, d)[d], face_offset(bc, d))
    return lo & hi


def grad_subtract(v, p, res, bc, dx, acc=None, dtype=np.float64):
    """ v_d - h * ((p_R - p_L) * (1 / dx_d)). Returns ([value_d], [S_d]) """
    T = np.dtype(dtype).type
    vals, scales = [], []
    for d in range(len(res)):
        pl, pr = _pressure_cells(np.asarray(p, T), d, res, bc)
        h = np.ones((1,) * pl.ndim, np.uint8) if acc is None else accessible_faces(acc, d, res, bc)
        g = (pr - pl) * T(1.0 / dx[d])
        vd = np.asarray(v[d], T)
        out = vd - h.astype(T) * g
        assert out.dtype == T
        vals.append(out)
        scales.append(np.abs(vd.astype(np.float64)) + h * (np.abs(pr.astype(np.float64)) + np.abs(pl.astype(np.float64))) * abs(1.0 / dx[d]))
    return vals, scales


# ---- masked Laplace --------------------------------------------------------------------------------------------------------------------------------------------
def masked_laplace(p, res, bc, dx, acc=None, active=None, dtype=np.float64):
    """ div(hard_bcs * grad p), identity on inactive cells. Without masks (acc is None and active is None) the flux form of the kernels without cell flags:
    ((p_hi - c) - (c - p_lo)) * w per axis, the axes summed from the slowest on; with masks the sum over the open faces of (neighbour - c) * w in the order lower,
    upper per axis, from 0. w_d = 1 / dx_d^2 rounded once. A face at a CLOSED side carries no flux, outside an OPEN side lies a zero ghost. Returns (value, S) """
    T = np.dtype(dtype).type
    D = len(res)
    c = np.asarray(p, T)
    c64 = np.abs(c.astype(np.float64))
    flagged = acc is not None or active is not None
    a = np.ones((1,) + tuple(res), np.uint8) if acc is None else (np.asarray(acc) != 0).astype(np.uint8)
    out = np.zeros_like(c) if flagged else None
    S = np.zeros(c.shape, np.float64)
    for d in range(D):
        ax = d + 1
        w = T(1.0 / (dx[d] * dx[d]))
        kinds = [WRAP if bc[d][s] == PERIODIC else CONST for s in (0, 1)]
        lo, hi = (x[_sl(c.ndim, ax, k, k + res[d])] for x, k in ((_ghost(c, ax, *kinds), 0), (_ghost(c, ax, *kinds), 2)))
        ag = _ghost(a, ax, *kinds, int(bc[d][0] == OPEN), int(bc[d][1] == OPEN))
        h_lo = a & ag[_sl(a.ndim, ax, 0, res[d])]
        h_hi = a & ag[_sl(a.ndim, ax, 2, res[d] + 2)]
        if flagged:
            out = np.where(h_lo > 0, out + (lo - c) * w, out)
            out = np.where(h_hi > 0, out + (hi - c) * w, out)
        else:           # (a closed face: the neighbour is the cell itself, both differences vanish exactly)
            term = (np.where(h_hi > 0, hi - c, T(0)) - np.where(h_lo > 0, c - lo, T(0))) * w
            out = term if out is None else out + term
        S += (h_hi * (np.abs(hi.astype(np.float64)) + c64) + h_lo * (np.abs(lo.astype(np.float64)) + c64)) / (dx[d] * dx[d])
    if flagged:
        act = a if active is None else a & (np.asarray(active) != 0).astype(np.uint8)
        act = np.broadcast_to(act, c.shape)
        out = np.where(act > 0, out, c)
        S = np.where(act > 0, S, c64)
    assert out.dtype == T
    return out, S


def cell_flags(acc, active, res, bc, batch_axis):
    """ packed cell flags: bit 2 a + side (a = d + 3 - D) = the face of the cell on that side is open (both cells accessible; outside: wrap / OPEN 1 / CLOSED 0),
    bit 6 = accessible and active. acc, active: bytes of ANY value (non-zero = set), with a leading batch axis when batch_axis """
    D = len(res)
    lead = 1 if batch_axis else 0
    a = np.ones(tuple(res), np.uint8) if acc is None else (np.asarray(acc) != 0).astype(np.uint8)
    out = np.zeros(a.shape, np.uint8)
    for d in range(D):
        ax = d + lead
        g = _ghost(a, ax, WRAP if bc[d][0] == PERIODIC else CONST, WRAP if bc[d][1] == PERIODIC else CONST, int(bc[d][0] == OPEN), int(bc[d][1] == OPEN))
        for side in (0, 1):
            other = g[_sl(a.ndim, ax, 2 * side, 2 * side + res[d])]
            out |= ((a & other) << (2 * (d + 3 - D) + side)).astype(np.uint8)
    act = a if active is None else a & (np.asarray(active) != 0).astype(np.uint8)
    return out | (act << 6).astype(np.uint8)


# ---- safe_mul, resample, diffusion ---------------------------------------------------------------------------------------------------------------------------------
def safe_mul(m, x, dtype=np.float64):
    """ m * x with 0 * anything = 0. Returns (value, S) """
    T = np.dtype(dtype).type
    m, x = np.asarray(m, T), np.asarray(x, T)
    with np.errstate(invalid='ignore', over='ignore'):
        out = np.where(m == 0, T(0), m * x)
        S = np.where(m == 0, 0.0, np.abs(m.astype(np.float64) * x.astype(np.float64)))
    return out, S


def _scalar_kind(code):
    return WRAP if code == PERIODIC else (CONST if code == CLOSED else EDGE)


def centered_to_staggered(s, res, bc, s_codes, s_consts, vector, base=None, dtype=np.float64):
    """ per component d: (s_L * vec_d) * 0.5 + (s_R * vec_d) * 0.5 at the stored faces, cells outside from the scalar's own rule; base: accumulate (base_d + value;
    a component whose vec_d is 0 stays as it is, bit for bit). Returns ([value_d], [S_d]) """
    T = np.dtype(dtype).type
    vals, scales = [], []
    for d in range(len(res)):
        ax = d + 1
        x = np.asarray(s, T)
        g = _ghost(x, ax, _scalar_kind(s_codes[d][0]), _scalar_kind(s_codes[d][1]), T(s_consts[d][0]), T(s_consts[d][1]))
        sl, sr = _two(g, ax, comp_shape(res, bc, d)[d], face_offset(bc, d))
        sc = T(vector[d])
        val = (sl * sc) * T(0.5) + (sr * sc) * T(0.5)
        S = abs(float(vector[d])) * 0.5 * (np.abs(sl.astype(np.float64)) + np.abs(sr.astype(np.float64)))
        if base is not None:
            b = np.asarray(base[d], T)
            val, S = (b, np.abs(b.astype(np.float64))) if float(vector[d]) == 0.0 else (b + val, S + np.abs(b.astype(np.float64)))
        assert val.dtype == T
        vals.append(val)
        scales.append(S)
    return vals, scales


def diffuse_explicit(v, res, bc, bcv, dx, kdt, dtype=np.float64):
    """ v_d + sum_a ((hi - c) - (c - lo)) * (kdt / dx_a^2) on the lattice of every component, neighbours outside from the velocity's own rule (wrap, edge sample,
    wall constant bcv[a][side][d]). Returns ([value_d], [S_d]) """
    T = np.dtype(dtype).type
    D = len(res)
    bcv = np.asarray(bcv, np.float64)
    vals, scales = [], []
    for d in range(D):
        c = np.asarray(v[d], T)
        c64 = np.abs(c.astype(np.float64))
        acc, S = None, c64.copy()
        for a in range(D):
            ax = a + 1
            n = c.shape[ax]
            g = _ghost(c, ax, _vel_kind(bc[a][0]), _vel_kind(bc[a][1]), T(bcv[a][0][d]), T(bcv[a][1][d]))
            lo, hi = g[_sl(c.ndim, ax, 0, n)], g[_sl(c.ndim, ax, 2, n + 2)]
            term = ((hi - c) - (c - lo)) * T(kdt / (dx[a] * dx[a]))
            acc = term if acc is None else acc + term
            S += (np.abs(hi.astype(np.float64)) + 2.0 * c64 + np.abs(lo.astype(np.float64))) * abs(kdt / (dx[a] * dx[a]))
        out = c + acc
        assert out.dtype == T
        vals.append(out)
        scales.append(S)
    return vals, scales


# ---- obstacles -------------------------------------------------------------------------------------------------------------------------------------------------
class Box:
    def __init__(self, lower, upper, rotation=None, velocity=None, angular_velocity=None):
        self.lower, self.upper, self.rotation, self.velocity, self.angular_velocity = tuple(lower), tuple(upper), rotation, velocity, angular_velocity

    @property
    def center(self):
        return tuple(0.5 * (l + u) for l, u in zip(self.lower, self.upper))

    def _local_excess(self, pts):
        """ |R^T (x - centre)| - half size per box axis """
        r = [p - c for p, c in zip(pts, self.center)]
        if self.rotation is not None:
            R = np.asarray(self.rotation, np.float64)
            r = [sum(R[c][a] * r[c] for c in range(len(r))) for a in range(len(r))]
        return [np.abs(x) - 0.5 * (u - l) for x, l, u in zip(r, self.lower, self.upper)]

    def lies_inside(self, pts):
        ok = np.ones(np.broadcast(*pts).shape, bool)
        for e in self._local_excess(pts):
            ok = ok & (e <= 0)
        return ok

    def sdf(self, pts):
        out = None
        for e in self._local_excess(pts):
            out = e if out is None else np.maximum(out, e)
        return out

    def surfaces(self, pts):
        return [self.sdf(pts)]

    @property
    def reach(self):
        return sum(abs(c) + 0.5 * (u - l) for c, l, u in zip(self.center, self.lower, self.upper))


class Sphere:
    def __init__(self, center, radius, velocity=None, angular_velocity=None):
        self.center, self.radius, self.velocity, self.angular_velocity = tuple(center), float(radius), velocity, angular_velocity

    def _d2(self, pts):
        return sum((p - c) * (p - c) for p, c in zip(pts, self.center))

    def lies_inside(self, pts):
        return self._d2(pts) <= self.radius * self.radius

    def sdf(self, pts):
        return np.sqrt(self._d2(pts)) - self.radius

    def surfaces(self, pts):
        return [self.sdf(pts)]

    @property
    def reach(self):
        return sum(abs(c) for c in self.center) + self.radius


class Embedded:
    """ a geometry of lower rank evaluated on the coordinates of `axes`, infinitely long along the others """
    def __init__(self, inner, axes, velocity=None):
        self.inner, self.axes, self.velocity, self.angular_velocity = inner, tuple(axes), velocity, None

    def lies_inside(self, pts):
        return self.inner.lies_inside([pts[a] for a in self.axes]) & np.ones(np.broadcast(*pts).shape, bool)

    def sdf(self, pts):
        return self.inner.sdf([pts[a] for a in self.axes]) + np.zeros(np.broadcast(*pts).shape)

    def surfaces(self, pts):
        return [self.sdf(pts)]

    @property
    def reach(self):
        return self.inner.reach


class Union:
    """ inside = any member, signed distance = the smallest; one linear velocity for the whole body """
    def __init__(self, members, velocity=None):
        self.members, self.velocity, self.angular_velocity = tuple(members), velocity, None

    def lies_inside(self, pts):
        out = self.members[0].lies_inside(pts)
        for m in self.members[1:]:
            out = out | m.lies_inside(pts)
        return out

    def sdf(self, pts):
        out = self.members[0].sdf(pts)
        for m in self.members[1:]:
            out = np.minimum(out, m.sdf(pts))
        return out

    def surfaces(self, pts):
        return [m.sdf(pts) for m in self.members]

    @property
    def reach(self):
        return max(m.reach for m in self.members)


def cell_points(res, lower, dx):
    D = len(res)
    return [(lower[a] + (np.arange(res[a]) + 0.5) * dx[a]).reshape([-1 if k == a else 1 for k in range(D)]) for a in range(D)]


def face_points(d, res, bc, lower, dx):
    D = len(res)
    shape = comp_shape(res, bc, d)
    pts = []
    for a in range(D):
        x = lower[a] + (np.arange(shape[a]) + (face_offset(bc, d) if a == d else 0.5)) * dx[a]
        pts.append(x.reshape([-1 if k == a else 1 for k in range(D)]))
    return pts


def accessible(obstacles, res, lower, dx):
    """ uint8 [*res]: 1 where the cell centre lies in no obstacle (lies_inside is inclusive) """
    pts = cell_points(res, lower, dx)
    inside = np.zeros(tuple(res), bool)
    for ob in obstacles:
        inside |= ob.lies_inside(pts)
    return (~inside).astype(np.uint8)


def surface_clearance(obstacles, res, bc, lower, dx):
    """ smallest distance, in units of the smallest cell size, between a sample position (cell centres, faces of every component) and the surface of any
    primitive: the discrete decision `inside` is safe from rounding where this is large against eps(float64) """
    h = min(dx)
    worst = np.inf
    sets = [cell_points(res, lower, dx)] + [face_points(d, res, bc, lower, dx) for d in range(len(res))]
    for pts in sets:
        for ob in obstacles:
            for s in ob.surfaces(pts):
                worst = min(worst, float(np.abs(s).min()) / h)
    return worst


def apply_obstacles(v, obstacles, res, bc, lower, dx, dtype=np.float64):
    """ per obstacle, in order: mask = clip(1 - sdf(face) / |half a cell's diagonal|, 0, 1) in float64, rounded once;
    v = safe_mul(1 - mask, v) [+ safe_mul(mask, angular_velocity x (x - centre) + velocity), the obstacle's velocity in float64 rounded once].
    Returns ([value_d], [E_d], [G_d]): E_d in units of eps of the element type, E_k = keep E_{k-1} + S_{k-1} + (moving: 1.5 m |u| + 0.5 S_k), S_k = keep S_{k-1} + m |u|
    (rounding of the mask: m / 2, of keep: keep / 2, of the product: keep / 2, together <= S_{k-1}; moving: mask, (T)u, the product: 3/2 m |u|, the sum: S_k / 2);
    G_d in units of eps(float64): the float64 geometry itself -- positions, differences, the rotation, the distance, 1 - sdf / radius carry a few eps64 of
    X = sum_a |x_a| + |centre_a| + |half size|, i.e. the mask X / radius, the velocity U = sum |w| |x - c| + |v|:
    G_k = keep G_{k-1} + X / radius (S_{k-1} + moving U) + moving m U (what decides an fp64 sample; 1e-9 of an fp32 bound) """
    T = np.dtype(dtype).type
    D = len(res)
    radius = float(np.sqrt(sum((0.5 * h) ** 2 for h in dx)))
    vals, errs, geos = [], [], []
    for d in range(D):
        pts = face_points(d, res, bc, lower, dx)
        val = np.asarray(v[d], T).copy()
        with np.errstate(invalid='ignore'):
            S = np.abs(val.astype(np.float64))
        E = np.zeros(val.shape, np.float64)
        G = np.zeros(val.shape, np.float64)
        for ob in obstacles:
            X = (sum(np.abs(p) for p in pts) + ob.reach)[None] / radius
            m64 = np.clip(1.0 - ob.sdf(pts) / radius, 0.0, 1.0)[None]
            m = m64.astype(T)
            keep = T(1) - m
            with np.errstate(invalid='ignore', over='ignore'):
                val = safe_mul(keep, val, T)[0]
                E = np.where(m64 >= 1.0, 0.0, (1.0 - m64) * E + np.where(m64 > 0, S, 0.0))
                G = (1.0 - m64) * G + X * np.where(np.isfinite(S), S, 0.0)
                S = np.where(m64 >= 1.0, 0.0, (1.0 - m64) * S)
            lin = ob.velocity if ob.velocity is not None else (0.0,) * D
            ang = ob.angular_velocity if ob.angular_velocity is not None else 0.0
            spins = bool(np.any(np.asarray(ang, np.float64) != 0))
            if any(float(c) != 0 for c in lin) or spins:
                u = np.zeros(np.broadcast(*pts).shape)
                U = np.zeros(np.broadcast(*pts).shape) + abs(float(lin[d]))
                if spins:
                    r = [pts[a] - ob.center[a] for a in range(D)]
                    U = U + float(np.abs(np.asarray(ang, np.float64)).max()) * sum(np.abs(p) + abs(c) for p, c in zip(pts, ob.center))
                    if D == 2:
                        w = float(np.asarray(ang, np.float64).reshape(-1)[0])
                        u = u + (-w * r[1], w * r[0])[d]
                    else:
                        w = np.broadcast_to(np.asarray(ang, np.float64), (3,))
                        u = u + (w[1] * r[2] - w[2] * r[1], w[2] * r[0] - w[0] * r[2], w[0] * r[1] - w[1] * r[0])[d]
                u = (u + float(lin[d]))[None]
                val = val + safe_mul(m, np.broadcast_to(u.astype(T), val.shape), T)[0]
                mu = m64 * np.abs(u)
                S = S + mu
                E = E + 1.5 * mu + 0.5 * S
                G = G + (X + m64) * U[None]
        assert val.dtype == T
        vals.append(val)
        errs.append(E)
        geos.append(G)
    return vals, errs, geos

"""
NumPy restatement (fp64) of diffusion with a spatially varying / per-axis diffusivity on a centred grid -- the reference's conservative
flux form (phi/physics/diffuse.py:129-141) as the issue states it, written out independently of the library and of oracle/:

    face_a = stagger(amount, math.minimum, NONE)     a_f = min(w a_L, w a_R) on all n + 1 faces, ghosts from the AMOUNT's extrapolation
    du     = u.gradient(boundary=NONE, at='face')    u_R - u_L, ghosts from u's extrapolation
    lap    = (face_a * du).divergence()              F_{i+1/2} - F_{i-1/2}

with w_d = k_d dt' / dx_d^2 signed. On an axis where u is periodic the end faces are one face between the last and the first cell.
Codes: 0 PERIODIC, 1 CLOSED (constant), 2 OPEN (zero-gradient) -- phihip.h PHIHIP_BC_*.

`lap` takes an element type: the same arithmetic in float32 is the yardstick of the fp32 kernels (tests/diffuse_coef_elementwise_cases.py).
`cg_trajectory` restates the first K iterations of diffuse.implicit's CG ('CG' and 'CG-adaptive': the recurrences of oracle/phi_oracle.py cg / cg_adaptive,
to which the cases module pins it) on  y = u - L(0),  A x = x + L_hom x,  x0 = u.  Imports nothing under test.
"""
from collections import namedtuple

import numpy as np

PERIODIC, CLOSED, OPEN = 0, 1, 2


def _ghosts(x, ax, code_lo, code_hi, c_lo, c_hi, wrap=False):
    """ x padded by one ghost layer on each side of tensor axis `ax` """
    n = x.shape[ax]
    first, last = np.take(x, [0], axis=ax), np.take(x, [n - 1], axis=ax)
    if wrap or code_lo == PERIODIC:
        lo, hi = last, first
    else:
        lo = first if code_lo == OPEN else np.full_like(first, c_lo)
        hi = last if code_hi == OPEN else np.full_like(last, c_hi)
    return np.concatenate([lo, x, hi], axis=ax)


def lap(u, a, w, u_codes, u_vals, a_codes=None, a_vals=None, dtype=np.float64):
    """ L_a u for u [B, *S]; a [Ba, *S] or None (1 everywhere); w[d] signed weights per spatial axis; every operation in `dtype` """
    T = np.dtype(dtype).type
    u = np.asarray(u, T)
    B, D = u.shape[0], u.ndim - 1
    if a is None:       # no coefficient array: 1 everywhere, ghosts included
        a, a_codes, a_vals = np.ones((1,) + u.shape[1:], T), [[OPEN, OPEN]] * D, [[0.0, 0.0]] * D
    a = np.broadcast_to(np.asarray(a, T), u.shape)
    w = [T(x) for x in w]
    out = np.zeros_like(u)
    for d in range(D):
        ax = d + 1
        uper = u_codes[d][0] == PERIODIC
        ue = _ghosts(u, ax, u_codes[d][0], u_codes[d][1], u_vals[d][0], u_vals[d][1])
        ae = _ghosts(a, ax, a_codes[d][0], a_codes[d][1], a_vals[d][0], a_vals[d][1], wrap=uper)
        n = u.shape[ax]
        sl = lambda i, j: tuple(slice(i, j) if k == ax else slice(None) for k in range(u.ndim))
        f = np.minimum(w[d] * ae[sl(0, n + 1)], w[d] * ae[sl(1, n + 2)])
        F = f * (ue[sl(1, n + 2)] - ue[sl(0, n + 1)])
        out += F[sl(1, n + 1)] - F[sl(0, n)]
    assert out.dtype == T
    return out


def explicit(u, a, kdt, dx, u_codes, u_vals, a_codes=None, a_vals=None, substeps=1, dtype=np.float64):
    """ kdt[d] = k_d * dt (total); substeps explicit Euler steps """
    w = [k / substeps / (h * h) for k, h in zip(kdt, dx)]
    u = np.asarray(u, dtype)
    for _ in range(substeps):
        u = u + lap(u, a, w, u_codes, u_vals, a_codes, a_vals, dtype)
    return u


def sharpen_matrix(shape, a, kdt, dx, u_codes, a_codes=None, a_vals=None):
    """ sparse matrix of the linear part x -> x + L_{-kdt} x (homogeneous walls) of ONE batch entry """
    import scipy.sparse as sp
    n = int(np.prod(shape))
    w = [-k / (h * h) for k, h in zip(kdt, dx)]
    zero = [[0.0, 0.0] for _ in shape]
    cols = []
    for i in range(n):
        e = np.zeros((1, n))
        e[0, i] = 1.0
        e = e.reshape((1,) + tuple(shape))
        cols.append((e + lap(e, a, w, u_codes, zero, a_codes, a_vals)).reshape(-1))
    return sp.csr_matrix(np.stack(cols, axis=1))


def implicit(y, a, kdt, dx, u_codes, u_vals, a_codes=None, a_vals=None):
    """ direct solve of sharpen(x) = y, sharpen(x) = x + L_{-kdt} x (affine walls moved to the right-hand side); a [Ba, *S] or None """
    import scipy.sparse.linalg as spl
    y = np.asarray(y, np.float64)
    w = [-k / (h * h) for k, h in zip(kdt, dx)]
    out = np.empty_like(y)
    for b in range(y.shape[0]):
        ab = None if a is None else np.asarray(a)[min(b, np.asarray(a).shape[0] - 1)][None]
        M = sharpen_matrix(y.shape[1:], ab, kdt, dx, u_codes, a_codes, a_vals)
        bias = lap(np.zeros((1,) + y.shape[1:]), ab, w, u_codes, u_vals, a_codes, a_vals).reshape(-1)
        out[b] = spl.spsolve(M.tocsc(), y[b].reshape(-1) - bias).reshape(y.shape[1:])
    return out


def implicit_residual(x, y, a, kdt, dx, u_codes, u_vals, a_codes=None, a_vals=None):
    """ per batch entry ||sharpen(x) - y|| / ||y - sharpen(0)|| in fp64 (the solve's own relative residual) """
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = [-k / (h * h) for k, h in zip(kdt, dx)]
    a = None if a is None else np.asarray(a, np.float64)
    r = x + lap(x, a, w, u_codes, u_vals, a_codes, a_vals) - y
    bias = lap(np.zeros_like(y), a, w, u_codes, u_vals, a_codes, a_vals)
    rhs = y - bias
    axes = tuple(range(1, y.ndim))
    return np.sqrt((r ** 2).sum(axis=axes) / (rhs ** 2).sum(axis=axes))


Trajectory = namedtuple("Trajectory", "x iterations residual_sq rhs_sq r y")


def cg_trajectory(u, a, kdt, dx, u_codes, u_vals, a_codes, a_vals, K, refresh_every, method='CG', dtype=np.float64):
    """ K iterations of diffuse.implicit's CG from x0 = u on  A x = x + L_hom x = y,  y = u - L(0)  (L(0): u's wall constants as ghosts of a zero field;
    L_hom: constants zero), w_d = -kdt_d / dx_d^2. method 'CG': alpha = r.r / d.q, beta = r'.r' / r.r; 'CG-adaptive': alpha = d.r / d.q, beta = -r'.q / d.q;
    on iteration k with k % refresh_every == 0 the residual is the true one, y - A x. Vectors in `dtype`, inner products in float64, per batch entry.
    Returns x, iterations [B], residual_sq [B] = sum r^2, rhs_sq [B] = sum y^2 and the vectors r and y """
    assert method in ('CG', 'CG-adaptive')
    T = np.dtype(dtype).type
    u = np.asarray(u, T)
    w = [-k / (h * h) for k, h in zip(kdt, dx)]
    zero = [[0.0, 0.0] for _ in w]
    A = lambda x: x + lap(x, a, w, u_codes, zero, a_codes, a_vals, dtype)
    dot = lambda p, q: (p.astype(np.float64) * q.astype(np.float64)).reshape(p.shape[0], -1).sum(axis=1)
    per = lambda s, v: np.asarray(s, np.float64).astype(T).reshape((-1,) + (1,) * (v.ndim - 1))
    div = lambda p, q: np.where(q != 0, p / np.where(q != 0, q, 1.0), 0.0)
    y = u - lap(np.zeros_like(u), a, w, u_codes, u_vals, a_codes, a_vals, dtype)
    x = u.copy()
    r = y - A(x)
    d = r.copy()
    rsq = dot(r, r)
    for k in range(1, int(K) + 1):
        q = A(d)
        dq = dot(d, q)
        alpha = div(rsq if method == 'CG' else dot(d, r), dq)
        x = x + per(alpha, x) * d
        r = y - A(x) if (refresh_every > 0 and k % refresh_every == 0) else r - per(alpha, r) * q
        rsq_old, rsq = rsq, dot(r, r)
        beta = div(rsq, rsq_old) if method == 'CG' else -div(dot(r, q), dq)
        d = r + per(beta, d) * d
        assert x.dtype == T and r.dtype == T and d.dtype == T
    return Trajectory(x, np.full(u.shape[0], int(K)), rsq, dot(y, y), r, y)

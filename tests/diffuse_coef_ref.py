"""
NumPy restatement (fp64) of diffusion with a spatially varying / per-axis diffusivity on a centred grid -- the reference's conservative
flux form (phi/physics/diffuse.py:129-141) as the issue states it, written out independently of the library and of oracle/:

    face_a = stagger(amount, math.minimum, NONE)     a_f = min(w a_L, w a_R) on all n + 1 faces, ghosts from the AMOUNT's extrapolation
    du     = u.gradient(boundary=NONE, at='face')    u_R - u_L, ghosts from u's extrapolation
    lap    = (face_a * du).divergence()              F_{i+1/2} - F_{i-1/2}

with w_d = k_d dt' / dx_d^2 signed. On an axis where u is periodic the end faces are one face between the last and the first cell.
Codes: 0 PERIODIC, 1 CLOSED (constant), 2 OPEN (zero-gradient) -- phihip.h PHIHIP_BC_*.
"""
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


def lap(u, a, w, u_codes, u_vals, a_codes=None, a_vals=None):
    """ L_a u for u [B, *S]; a [Ba, *S] or None (1 everywhere); w[d] signed weights per spatial axis """
    u = np.asarray(u, np.float64)
    B, D = u.shape[0], u.ndim - 1
    if a is None:       # no coefficient array: 1 everywhere, ghosts included
        a, a_codes, a_vals = np.ones((1,) + u.shape[1:]), [[OPEN, OPEN]] * D, [[0.0, 0.0]] * D
    a = np.broadcast_to(a, u.shape)
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
    return out


def explicit(u, a, kdt, dx, u_codes, u_vals, a_codes=None, a_vals=None, substeps=1):
    """ kdt[d] = k_d * dt (total); substeps explicit Euler steps """
    w = [k / substeps / (h * h) for k, h in zip(kdt, dx)]
    u = np.asarray(u, np.float64)
    for _ in range(substeps):
        u = u + lap(u, a, w, u_codes, u_vals, a_codes, a_vals)
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

"""
TEST INFRASTRUCTURE: a plain float64 restatement, in NumPy and scipy.sparse, of the multigrid V-cycle that preconditions
Solve(..., preconditioner='multigrid') (csrc/multigrid.hpp, DESIGN.md "f6"), and of the preconditioned CG recurrence around it. It restates the
RECIPE of that header, not the kernels' loops, and imports nothing that is under test:

  fine operator  P = -A on the active cells, assembled as a sparse matrix from the oracle's masks (O.obstacle_masks' hard face mask and active cells),
                 the domain's boundary codes and 1 / dx^2 per axis: every open face adds w to the diagonal of the active cells it touches and -w to
                 the coupling of two ACTIVE cells; inactive neighbours and OPEN walls are zero ghosts (diagonal only), CLOSED walls carry no flux.
                 A flagged-active cell whose diagonal is zero (a one-cell pocket) counts as inactive. `pin` ties P to O.masked_laplace.
  hierarchy      n -> ceil(n / 2) per axis until the smallest axis has <= coarsest_cells cells (16 levels at most). R = child-sum matrix over the
                 ACTIVE children; the coarse operator is the explicit sparse Galerkin product R P R^T -- the kernels keep a diagonal and one coupling
                 array per axis and book-keep inner and outer faces instead. A coarse cell is active iff its diagonal exceeds 1e-4 x the sum of its
                 children's diagonals; rows and columns of inactive cells are zeroed.
  cycle          damped Jacobi x <- x + omega (b - P x) / d, the first sweep from zero (x = omega b / d); nu sweeps, b_c = R (b - P x), recursion,
                 x += 2 R^T e, nu sweeps; the coarsest level (and a single-level hierarchy) runs 2 x bottom sweeps from zero.
                 z = -x on active cells, z = r on inactive cells.
  PCG            r = y - A x0; per iteration z = M r, beta = r.z / (r.z)_old (0 in the first), d = z + beta d, alpha = r.z / d.Ad, x += alpha d,
                 r -= alpha A d, or r = y - A x when k % refresh_every == 0. A is the ORACLE's masked_laplace, M this cycle.

`dtype=np.float32` runs the identical arithmetic in float32: the fine matrix is cast, the Galerkin products, every sweep and every transfer stay in float32. Its
distance from the float64 run on the same inputs is the yardstick of the fp32 kernels (tests/multigrid_elementwise_cases.py). The inner products of
the PCG reference are summed in float64 whatever the element type, as the documented recurrence keeps its scalars in double.

Not covered: a PERIODIC axis of ONE cell on the fine level (the matrix folds the cell's coupling with itself into a zero diagonal, the fine-level kernels
count both faces); no case uses one.
"""
import numpy as np
import scipy.sparse as sp

from oracle import phi_oracle as O

PER, CLO, OPN = O.PERIODIC, O.CLOSED, O.OPEN
MAX_LEVELS = 16
ACTIVE_THRESHOLD = 1e-4


def fine_operator(dom, hard=None, active=None):
    """ (P, act): P = -masked_laplace restricted to the active cells as a float64 CSR matrix over ALL cells (zero rows and columns elsewhere), act = the
    cells that are flagged active AND have a non-zero diagonal (flat bool). hard: the oracle's face masks per axis or None (every stored face open);
    active: (1, *res) or None """
    res, D = dom.res, dom.rank
    N = int(np.prod(res))
    idx = np.arange(N).reshape(res)
    flagged = np.ones(N, bool) if active is None else (np.asarray(active).reshape(-1) > 0)
    rows, cols, vals = [], [], []

    def entry(i, j, v):
        rows.append(i)
        cols.append(j)
        vals.append(np.full(len(i), v))

    for d in range(D):
        n = res[d]
        w = 1.0 / dom.dx[d] ** 2
        H = np.ones(dom.comp_shape(d)) if hard is None else np.asarray(hard[d], np.float64).reshape(dom.comp_shape(d))
        off = dom.face_offset(d)                       # physical face k (between the cells k - 1 and k) is stored at k - off
        cells = lambda k: np.take(idx, k, axis=d).ravel()
        faces = lambda k: np.take(H, k, axis=d).ravel() > 0

        def between(i, j, is_open):
            ai, aj = is_open & flagged[i], is_open & flagged[j]
            entry(i[ai], i[ai], w)
            entry(j[aj], j[aj], w)
            both = ai & aj
            entry(i[both], j[both], -w)
            entry(j[both], i[both], -w)

        def ghost(i, is_open):
            a = is_open & flagged[i]
            entry(i[a], i[a], w)

        if n > 1:
            k = np.arange(1, n)
            between(cells(k - 1), cells(k), faces(k - off))
        lo, hi = dom.bc[d]
        if lo == PER:
            between(cells([n - 1]), cells([0]), faces([0]))
        else:
            if lo == OPN:
                ghost(cells([0]), faces([0]))
            if hi == OPN:
                ghost(cells([n - 1]), faces([n - off]))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()   # (duplicates are summed)
    P.eliminate_zeros()
    act = flagged & (P.diagonal() > 0)
    return P, act


class Level:
    def __init__(self, P, act, shape):
        self.P, self.act, self.shape = P, act, tuple(shape)
        self.d = P.diagonal()
        self.dsafe = np.where(act, self.d, self.d.dtype.type(1))
        self.R = None      # child-sum matrix towards the next level


class Hierarchy:
    """ the levels of one geometry for one `coarsest_cells`, in `dtype` """

    def __init__(self, dom, hard=None, active=None, coarsest_cells=4, dtype=np.float64):
        self.dom, self.hard, self.active_mask, self.dtype = dom, hard, active, np.dtype(dtype)
        T = self.dtype.type
        P, act = fine_operator(dom, hard, active)
        self.P64 = P
        P = P.astype(self.dtype)
        shape = tuple(dom.res)
        stop = max(int(coarsest_cells), 1)
        self.levels = []
        while True:
            L = Level(P, act, shape)
            self.levels.append(L)
            if min(shape) <= stop or len(self.levels) == MAX_LEVELS:
                break
            cshape = tuple((n + 1) // 2 for n in shape)
            parent = np.ravel_multi_index(tuple(c >> 1 for c in np.indices(shape)), cshape).ravel()
            children = np.flatnonzero(act)
            R = sp.csr_matrix((np.ones(len(children), self.dtype), (parent[children], children)), shape=(int(np.prod(cshape)), len(parent)))
            Pc = (R @ P @ R.T).tocsr()
            actc = Pc.diagonal() > T(ACTIVE_THRESHOLD) * (R @ L.d)
            S = sp.diags(actc.astype(self.dtype))
            Pc = (S @ Pc @ S).tocsr()
            Pc.eliminate_zeros()
            assert Pc.dtype == self.dtype and R.dtype == self.dtype
            L.R = R
            P, act, shape = Pc, actc, cshape

    @property
    def nlevels(self):
        return len(self.levels)

    @property
    def active(self):
        """ the fine cells the cycle treats as active, shaped like the grid """
        return self.levels[0].act.reshape(self.dom.res)

    def _jacobi(self, L, b, x, omega):
        return np.where(L.act, x + omega * (b - L.P @ x) / L.dsafe, self.dtype.type(0))

    def _cycle(self, l, b, nu, bottom, omega):
        L = self.levels[l]
        zero = self.dtype.type(0)
        x = np.where(L.act, omega * b / L.dsafe, zero)
        if l == len(self.levels) - 1:
            for _ in range(2 * bottom - 1):
                x = self._jacobi(L, b, x, omega)
            return x
        for _ in range(nu - 1):
            x = self._jacobi(L, b, x, omega)
        e = self._cycle(l + 1, L.R @ (b - L.P @ x), nu, bottom, omega)
        x = x + self.dtype.type(2) * (L.R.T @ e)
        for _ in range(nu):
            x = self._jacobi(L, b, x, omega)
        return x

    def apply(self, r, sweeps=2, bottom=30, omega=0.8):
        """ z = M r for ONE batch entry, r shaped (*res) or (1, *res); the result has r's shape and the hierarchy's element type """
        r = np.asarray(r)
        b = r.reshape(-1).astype(self.dtype)
        x = self._cycle(0, b, int(sweeps), int(bottom), self.dtype.type(omega))
        z = np.where(self.levels[0].act, -x, b)
        assert z.dtype == self.dtype
        return z.reshape(r.shape)

    def A(self, x):
        """ the ORACLE's operator (identity on inactive cells) in x's element type; x shaped (1, *res) """
        return O.masked_laplace(x, self.dom, self.hard, self.active_mask)

    def pin(self, seeds=(101, 102), bound=1e-12):
        """ -P x = O.masked_laplace(x) on the active cells for random x (zero on inactive cells: P lives on the active ones), to `bound` of max |.| """
        worst = 0.0
        act = self.levels[0].act
        flagged = np.ones(act.shape, bool) if self.active_mask is None else (np.asarray(self.active_mask).reshape(-1) > 0)
        for seed in seeds:
            x = np.random.default_rng(seed).standard_normal(act.shape) * flagged
            ref = self.A(x.reshape((1,) + tuple(self.dom.res))).reshape(-1)
            got = -(self.P64 @ x)
            scale = max(float(np.abs(ref[flagged]).max()) if flagged.any() else 0.0, 1e-300)
            err = float(np.abs(got - ref)[flagged].max()) / scale if flagged.any() else 0.0
            worst = max(worst, err)
            assert err <= bound, f"the reference's fine operator is {err:.2e} of max|A x| from O.masked_laplace"
        return worst


class PcgResult(tuple):
    """ (x, sum r^2, iterations) with the residual and sum y^2 riding along """
    def __new__(cls, x, residual_sq, iterations, r, rhs_sq):
        self = super().__new__(cls, (x, residual_sq, iterations))
        self.x, self.residual_sq, self.iterations, self.r, self.rhs_sq = x, residual_sq, iterations, r, rhs_sq
        return self


def pcg(H, y, x0, iterations, refresh_every=50, sweeps=2, bottom=30, omega=0.8):
    """ `iterations` steps of CG on A x = y preconditioned by H's cycle, from x0; one batch entry shaped (1, *res). Vectors in H's element type, inner
    products in float64. Returns (x, sum r^2, iterations) """
    T = H.dtype.type
    dot = lambda a, b: float(np.sum(a.astype(np.float64) * b.astype(np.float64)))
    y = np.asarray(y).astype(H.dtype)
    x = np.asarray(x0).astype(H.dtype)
    r = y - H.A(x)
    rz_old, d = 0.0, None
    for k in range(1, int(iterations) + 1):
        z = H.apply(r, sweeps, bottom, omega)
        rz = dot(r, z)
        beta = rz / rz_old if (k > 1 and rz_old != 0) else 0.0
        d = z if k == 1 else z + T(beta) * d
        Ad = H.A(d)
        dAd = dot(d, Ad)
        alpha = rz / dAd if dAd != 0 else 0.0
        x = x + T(alpha) * d
        r = y - H.A(x) if (refresh_every > 0 and k % refresh_every == 0) else r - T(alpha) * Ad
        rz_old = rz
        assert x.dtype == H.dtype and r.dtype == H.dtype
    return PcgResult(x, dot(r, r), int(iterations), r, dot(y, y))

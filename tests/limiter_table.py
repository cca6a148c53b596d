"""
A hand-derived table of the MacCormack limiter, centred and staggered: literals only. Worked out on paper from the reference's definition
(phi/physics/advect.py:198-214: fwd = field(x - dt u), bwd = fwd(x + dt u), new = fwd + strength / 2 (field - bwd), clipped to the min / max of the grid values
around x - dt u; phi/field/_field.py:409-429: those are the values left and right of the point in the CELL grid's index frame, x / dx - 1/2, for every field),
NOT taken from the oracle or from tests/adjoint_ref.py. Used against the kernels (tests/advect_forward_cases.py check_limiter_table) and against the oracle
(tests/test_oracle_reference_pins.py). DESIGN.md "f11" shows the working.

The grid is (1, 8): one periodic cell along axis 0 and no velocity along it, so everything happens on the line of 8 cells along axis 1; dx = 1, dt = 1/2,
strength 1. Every weight is a multiple of 1/4 and every value a small dyadic number: the arithmetic is exact in fp32, the comparison is equality.
"""
RES = (1, 8)
DT = 0.5

# ---- centred scalar ------------------------------------------------------------------------------------------------------------------------------------------
# velocity: open line, 9 faces; centre velocity U_i = (w_i + w_{i+1}) / 2, displacement d_i = U_i / 2 cells
CEN_FACES = [0.5, 0.5, 0.5, 1.5, 1.5, -0.5, -0.5, -1.5, -1.5]
#        U = [0.5, 0.5, 1.0, 1.5, 0.5, -0.5, -1.0, -1.5]       d = [.25, .25, .5, .75, .25, -.25, -.5, -.75]
# scalar: constant 2 below the line (s[-1] = 2), open above (s[8] = s[7])
CEN_CONSTS = (2.0, 0.0)
CEN_S = [4.0, 4.0, 0.0, 8.0, 0.0, 0.0, 4.0, 8.0]
# backward points c_i = i - d_i = [-.25, .75, 1.5, 2.25, 3.75, 5.25, 6.5, 7.75]
CEN_BACK = [-0.25, 0.75, 1.5, 2.25, 3.75, 5.25, 6.5, 7.75]
#   fwd_0 = .25 * 2 + .75 * 4;  fwd_2 = (4 + 0) / 2;  fwd_3 = .75 * 0 + .25 * 8;  fwd_4 = .25 * 8 + .75 * 0;  fwd_5 = .25 * 4;  fwd_6 = (4 + 8) / 2;  fwd_7 = .25 * 8 + .75 * 8
CEN_FWD = [3.5, 4.0, 2.0, 2.0, 2.0, 1.0, 6.0, 8.0]
# forward points e_i = i + d_i = [.25, 1.25, 2.5, 3.75, 4.25, 4.75, 5.5, 6.25]; bwd_i = fwd(e_i)
#   bwd_0 = .75 * 3.5 + .25 * 4;  bwd_1 = .75 * 4 + .25 * 2;  bwd_4 = .75 * 2 + .25 * 1;  bwd_5 = .25 * 2 + .75 * 1;  bwd_6 = (1 + 6) / 2;  bwd_7 = .75 * 6 + .25 * 8
CEN_BWD = [3.625, 3.5, 2.0, 2.0, 1.75, 1.25, 3.5, 6.5]
CEN_NEW = [3.6875, 4.25, 1.0, 5.0, 1.125, 0.375, 6.25, 8.75]
# the values left and right of c_i: (2, 4) (4, 4) (4, 0) (0, 8) (8, 0) (0, 4) (4, 8) (8, 8)
CEN_LO = [2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 4.0, 8.0]
CEN_HI = [4.0, 4.0, 4.0, 8.0, 8.0, 4.0, 8.0, 8.0]
# sample 1 sits in a constant stretch and overshoots it, sample 7 overshoots the open end, sample 3 is the local extremum and keeps its corrected value
CEN_OUT = [3.6875, 4.0, 1.0, 5.0, 1.125, 0.375, 6.25, 8.0]

# ---- staggered component along the line ----------------------------------------------------------------------------------------------------------------------
# closed below (the wall face is the constant 2), open above: faces 1 .. 8 are stored, stored index k sits at x = k + 1. Field g and velocity w on those faces;
# displacement d_k = w_k / 2
STAG_WALL = 2.0
STAG_W = [0.5, 1.5, 0.5, -0.5, -1.5, 0.5, 1.5, -0.5]      # d = [.25, .75, .25, -.25, -.75, .25, .75, -.25]
STAG_G = [4.0, 0.0, 8.0, 0.0, 0.0, 4.0, 4.0, 8.0]         # g[-1] = 2 (wall), g[8] = g[7]
# backward points in the component's own index frame c_k = k - d_k = [-.25, .25, 1.75, 3.25, 4.75, 4.75, 5.25, 7.25]
STAG_FWD = [3.5, 3.0, 6.0, 0.0, 3.0, 3.0, 4.0, 8.0]
# forward points e_k = k + d_k = [.25, 1.75, 2.25, 2.75, 3.25, 5.25, 6.75, 6.75]
STAG_BWD = [3.375, 5.25, 4.5, 1.5, 0.75, 3.25, 7.0, 7.0]
STAG_NEW = [3.8125, 0.375, 7.75, -0.75, 2.625, 3.375, 2.5, 8.5]
# the limiter's window is taken in the CELL frame: m_k = x / dx - 1/2 = c_k + 1/2 = [.25, .75, 2.25, 3.75, 5.25, 5.25, 5.75, 7.75], values g[floor m], g[floor m + 1]:
#   (4, 0) (4, 0) (8, 0) (0, 0) (4, 4) (4, 4) (4, 4) (8, 8)            (the component's own frame would give (0, 4) at k = 4 and 5: results 2.625 and 3.375)
STAG_LIMIT_COORD = [0.25, 0.75, 2.25, 3.75, 5.25, 5.25, 5.75, 7.75]
STAG_LO = [0.0, 0.0, 0.0, 0.0, 4.0, 4.0, 4.0, 8.0]
STAG_HI = [4.0, 4.0, 8.0, 0.0, 4.0, 4.0, 4.0, 8.0]
STAG_OUT = [3.8125, 0.375, 7.75, 0.0, 4.0, 4.0, 4.0, 8.0]

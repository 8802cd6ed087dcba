"""NumPy restatement of dvs_pose_fit (csrc/posefit.hip; include/dvslam.h states the arithmetic) and the seeded inputs of its tests:
the camera motion under which a static scene of a given depth shows a measured flow, by Gauss-Newton on SE(3) with Huber weights.

    terms(...)            (a) the accumulate launch, operation by operation in fp32: the 30 per-pixel terms [N,30,H,W] and what leads
                          to them; with dtype=np.float64, (b), the same formulas in fp64 from the same fp32 inputs
    normal(t)             the terms of the judged pixels widened and summed in fp64: the row [N,30] the kernel hands out
    step(row, T, damping) the update launch in fp64: (T fp32 [4,4], taken)
    fit(...)              `iters` (terms, normal, step) rounds; (a) rounds T to fp32 after every step as the kernel does, (b) keeps
                          T in fp64 throughout

THE SUMMATION BOUND (kernel against (a)).  The kernel and (a) form the SAME fp32 terms (every operation is correctly rounded on both
sides, contraction is off) and differ in the order of the fp64 additions alone.  sum_bound() returns n 2^-53 sum|term| per entry:
the bound the issue sets, used as it stands.  What can be derived: a sum of n fp64 numbers whose summation tree has depth k (the
largest number of additions any term passes through) lies within k 2^-53 sum|term| of the exact sum to first order (Higham,
Accuracy and Stability, section 4.2), so two orders of depths k1 and k2 lie within (k1 + k2) 2^-53 sum|term| of each other.  The
kernel's depth is (pixels a lane owns) + 6 shuffle steps + 3 waves + (rows - 1); NumPy's is n - 1 below 8 terms and about
n / 8 + 3 + log2 above.  For n >= 24 judged pixels k1 + k2 <= n holds at every tested shape and the issue's bound is the derived one
or looser; for fewer terms k1 + k2 can reach 2 (n - 1) > n, and there the issue's bound is TIGHTER than what is derived -- it is
kept, not widened, and holds in the measurements (at most 0.12 of it).

THE fp32 BOUND ((a) against (b)), u = 2^-24, first order in u, |.| of a sum = the sum of the absolute values of its terms:

    r_i = iK[i][0] x + iK[i][1] y + iK[i][2]    |dr_i| <= 3 u R_i                         (rigidflow_ref)
    X_i = d r_i                                 |dX_i| <= 4 u A_i,  A_i = |d| R_i
    q_i = sum_j T[i][j] X_j + T[i][3]           a product: |T_ij| dX_j + u |T_ij X_j| <= 5 u |T_ij| A_j, and at most 3 sums:
                                                |dq_i| <= 8 u Q_i,  Q_i = sum_j |T_ij| A_j + |T_i3|
    c_i = sum_j K[i][j] q_j + K[i][3]           a product: |K_ij| dq_j + u |K_ij q_j| <= 9 u |K_ij| Q_j, at most 3 sums:
                                                |dc_i| <= 12 u C_i, C_i = sum_j |K_ij| Q_j + |K_i3|
    den = c_z + eps                             |dden| <= 12 u C_z + u |den|
    p = c / den                                 Ep = 12 u (C + |p| C_z) / |den| + 2 u |p|
    t = x + f                                   u |t|
    e = p - t                                   De = Ep + u |t| + u |e|
    n_rk = K[r][k] - p K[2][k]                  Dn = |K_2k| Ep + u |p K_2k| + u |n_rk|
    A_rk = n_rk / den                           DA = Dn / |den| + |A_rk| |dden| / |den| + u |A_rk|
    J_r3 = A_r2 q_y - A_r1 q_z  (and 4, 5)      DJ = sum over its two products (DA |q| + |A| 8 u Q + u |A q|) + u |J|
    e2 = ex^2 + ey^2                            De2 = 2 (|ex| Dex + |ey| Dey) + 2 u e2
    w = 1 or huber / sqrt(e2)                   Dw = 0 where e2 + De2 <= huber^2 (1 - 2 u): both sides take w = 1; elsewhere
                                                Dw = w (De2 / (2 e2) + 2 u): the slope of e2^-1/2, a sqrt and a quotient -- w is
                                                continuous across huber^2, so a pixel whose two sides take different branches is
                                                covered by the same expression
    h_ij = w (J_0i J_0j + J_1i J_1j)            w sum_r (DJ_ri |J_rj| + |J_ri| DJ_rj) + (3 u w + Dw) sum_r |J_ri J_rj|
    g_i  = w (J_0i ex + J_1i ey)                the same with e for J_j
    w e2                                        Dw e2 + w De2 + u w e2;      w: Dw;      1: 0

and an entry's bound is the sum of its terms' bounds over the judged pixels (the fp64 summation adds n 2^-53 sum|term|, which is
included).  The judged SETS of (a) and (b) must agree for the bound to mean anything; the seeded scenes keep every target away from
the border and every cz away from 0 (asserted by the test).

MEASURED (tests/test_posefit_cpu.py prints them):
    (a) against (b), the 30 sums: at most 0.13 of the bound (1x1; 0.02 at 131x77) over test_fp32_sums_against_fp64's shapes
    recovery of the fixture's T from the identity, max |T - T_fixture| over the scenes of RECOVERY after 6 steps:
        (b) 2.7e-07 (the fixture's own fp32 flow and T), (a) against (b) 1.22e-07, recorded as RECOVERY_A_VS_B = 1.3e-07; the
        kernel is allowed 4 x that against (b), RECOVERY_TOL: it differs from (a) by the fp64 summation order and by the last
        bits of sin, cos and sqrt in the update, each far below the fp32 rounding of T that (a) already carries.

This is a plain module (imported like rigidflow_ref), not a conftest.
"""
from types import SimpleNamespace

import numpy as np

import rigidflow_ref as R

F32 = np.float32
U = 2.0 ** -24
U64 = 2.0 ** -53
SUMS = 30
HUBER, DAMPING, EPS = 1.0, 1e-6, 1e-7
IDX = [(i, j) for i in range(6) for j in range(i, 6)]          # entry k < 21 of a row is H[i][j]
bits = R.bits


def _mats(m, N, T):
    m = np.asarray(m)
    assert m.shape in ((4, 4), (N, 4, 4)), m.shape
    return np.broadcast_to(m, (N, 4, 4)).astype(T)


def terms(depth, flow, K, iK, T, valid=None, huber=HUBER, eps=EPS, dtype=F32):
    """The accumulate launch.  depth [N,H,W] or [N,1,H,W], flow [N,2,H,W], K, iK [4,4] or [N,4,4] fp32; T [N,4,4] (fp32 for the
    restatement; fp64 is taken as it is by dtype=np.float64); valid uint8 [N,H,W] or None.  A namespace: term [N,30,H,W] in `dtype`
    (whatever it holds where judged is False is not summed), judged [N,H,W] bool, w, e2, ex, ey, px, py, cz, tx, ty, J [2][6]."""
    depth, flow = np.asarray(depth), np.asarray(flow)
    assert depth.dtype == F32 and flow.dtype == F32
    if depth.ndim == 4:
        depth = depth[:, 0]
    N, H, W = depth.shape
    assert flow.shape == (N, 2, H, W)
    Tt = dtype
    if Tt == F32:
        assert np.asarray(T).dtype == F32 and np.asarray(K).dtype == F32 and np.asarray(iK).dtype == F32
    T, K, iK = _mats(T, N, Tt), _mats(K, N, Tt), _mats(iK, N, Tt)
    at = lambda m, i, j: m[:, i, j][:, None, None]
    huber, eps = Tt(F32(huber)), Tt(F32(eps))
    with np.errstate(all="ignore"):
        x = np.arange(W, dtype=F32).astype(Tt)[None, None, :]
        y = np.arange(H, dtype=F32).astype(Tt)[None, :, None]
        d = depth.astype(Tt)
        r = [(at(iK, i, 0) * x + at(iK, i, 1) * y) + at(iK, i, 2) for i in range(3)]
        X = [d * r[i] for i in range(3)]
        q = [((at(T, i, 0) * X[0] + at(T, i, 1) * X[1]) + at(T, i, 2) * X[2]) + at(T, i, 3) for i in range(3)]
        c = [((at(K, i, 0) * q[0] + at(K, i, 1) * q[1]) + at(K, i, 2) * q[2]) + at(K, i, 3) for i in range(3)]
        den = c[2] + eps
        p = [c[0] / den, c[1] / den]
        fu, fv = flow[:, 0].astype(Tt), flow[:, 1].astype(Tt)
        tx, ty = x + fu, y + fv
        e = [p[0] - tx, p[1] - ty]
        judged = (np.isfinite(d) & (d > 0) & np.isfinite(fu) & np.isfinite(fv) & (c[2] > 0) & (tx >= 0) & (tx <= Tt(W - 1)) & (ty >= 0)
                  & (ty <= Tt(H - 1)) & np.isfinite(e[0]) & np.isfinite(e[1]))
        if valid is not None:
            valid = np.asarray(valid)
            assert valid.dtype == np.uint8 and valid.shape == (N, H, W)
            judged = judged & (valid != 0)
        e2 = e[0] * e[0] + e[1] * e[1]
        quadratic = e2 <= huber * huber
        w = np.where(quadratic, Tt(1), huber / np.sqrt(e2))
        J = []
        for k in range(2):
            a = [(at(K, k, m) - p[k] * at(K, 2, m)) / den for m in range(3)]
            J.append([a[0], a[1], a[2], a[2] * q[1] - a[1] * q[2], a[0] * q[2] - a[2] * q[0], a[1] * q[0] - a[0] * q[1]])
        term = [w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]) for i, j in IDX]
        term += [w * (J[0][i] * e[0] + J[1][i] * e[1]) for i in range(6)]
        term += [w * e2, w + 0 * e2, np.ones_like(e2)]
        term = np.stack([np.broadcast_to(t, (N, H, W)) for t in term], 1)
    assert term.dtype == Tt and term.shape == (N, SUMS, H, W) and w.dtype == Tt
    return SimpleNamespace(term=term, judged=np.broadcast_to(judged, (N, H, W)), quadratic=np.broadcast_to(quadratic, (N, H, W)),
                           w=w, e2=e2, ex=e[0], ey=e[1], px=p[0], py=p[1], cz=c[2], den=den, tx=tx, ty=ty, J=J, q=q, N=N, H=H, W=W)


def normal(t):
    """[N,30] fp64: the judged pixels' terms, widened and summed (NumPy's pairwise order)."""
    with np.errstate(all="ignore"):
        return np.where(t.judged[:, None], t.term.astype(np.float64), 0.0).reshape(t.N, SUMS, -1).sum(-1)


def abs_sum(t):
    """(sum|term| [N,30] fp64, n [N]) over the judged pixels."""
    with np.errstate(all="ignore"):
        a = np.where(t.judged[:, None], np.abs(t.term.astype(np.float64)), 0.0).reshape(t.N, SUMS, -1).sum(-1)
    return a, t.judged.reshape(t.N, -1).sum(-1)


def sum_bound(t):
    """n 2^-53 sum|term| per entry [N,30]: how far an fp64 sum of the same n terms in another order may lie (module docstring)."""
    a, n = abs_sum(t)
    return n[:, None] * U64 * a


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
CHOLESKY_OPS = 6 * 6 * 6 // 3 + 2 * 6 * 6          # c of the update test: n^3/3 for the factorisation, 2 n^2 for the two substitutions


def update_bound(row, xi, ref, T0):
    """(bound [4,4] on |T_kernel - ref|, kappa): ref = the fp64 update of posefit_ref on the kernel's own row, not yet rounded.

    Both sides run the same fp64 operations on the same row, so they differ by no more than the backward error of a 6x6 Cholesky
    solve allows, |dxi| <= kappa(A) c 2^-53 |xi| with c = CHOLESKY_OPS = 144 (Higham, theorem 10.4, first order), plus the last
    bits of sqrt, sin and cos, which enter the coefficients a, b, c (each at most 1 in magnitude) with at most 2 units of 2^-53
    each: s = 4 2^-53 per entry of exp(xi).  Through exp: an entry of R moves by at most |domega| <= |dxi|; t = V nu by at most
    |V| |dnu| + |dV| |nu| <= (1 + |xi|) |dxi| (|V| <= 1 + theta / 2, |dV| <= |domega|); so |dE| <= (1 + |xi|) (|dxi| + s) per
    entry.  T = E T0 sums four products: |dT| <= 4 (1 + |xi|) (|dxi| + s) max|T0|.  The result is then rounded to fp32, the
    nearest of which lies within 2^-24 |ref| of ref."""
    kappa = float(np.linalg.cond(system(row)[0]))
    n = float(np.linalg.norm(xi))
    dxi = kappa * CHOLESKY_OPS * U64 * n
    return U * np.abs(ref) + 4 * (1 + n) * (dxi + 4 * U64) * float(np.abs(T0).max()) + U * 2.0 ** -126, kappa


def system(row, damping=DAMPING):
    """(A [6,6], g [6]) of one row of 30 sums: A = H + damping diag(H)."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(IDX):
        A[i, j] = A[j, i] = row[k]
    damping = np.float64(F32(damping))
    for i in range(6):
        A[i, i] = A[i, i] + damping * A[i, i]
    return A, np.asarray(row[21:27], np.float64)


def solve(row, damping=DAMPING):
    """xi of one row, or None where the step is skipped: the kernel's Cholesky, operation by operation in fp64."""
    row = np.asarray(row, np.float64)
    if not row[29] >= 6.0 or not np.isfinite(row).all():
        return None
    A, g = system(row, damping)
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            p = A[j, j]
            for k in range(j):
                p = p - L[j, k] * L[j, k]
            if not p > 0.0:
                return None
            L[j, j] = np.sqrt(p)
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v = v - L[i, k] * L[j, k]
                L[i, j] = v / L[j, j]
        yv, xi = np.zeros(6), np.zeros(6)
        for i in range(6):
            v = -g[i]
            for k in range(i):
                v = v - L[i, k] * yv[k]
            yv[i] = v / L[i, i]
        for i in reversed(range(6)):
            v = yv[i]
            for k in range(i + 1, 6):
                v = v - L[k, i] * xi[k]
            xi[i] = v / L[i, i]
    return xi if np.isfinite(xi).all() else None


def exp_se3(xi):
    """[4,4] fp64: exp of xi = (nu, omega), the kernel's closed form and its series branch."""
    wx, wy, wz = xi[3], xi[4], xi[5]
    th2 = (wx * wx + wy * wy) + wz * wz
    if th2 < 1e-4:
        th4 = th2 * th2
        a, b, c = (1.0 - th2 / 6.0) + th4 / 120.0, (0.5 - th2 / 24.0) + th4 / 720.0, (1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0
    else:
        th = np.sqrt(th2)
        sn, cs = np.sin(th), np.cos(th)
        a, b, c = sn / th, (1.0 - cs) / th2, (th - sn) / (th2 * th)
    Wm = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    W2 = np.array([[(Wm[i, 0] * Wm[0, j] + Wm[i, 1] * Wm[1, j]) + Wm[i, 2] * Wm[2, j] for j in range(3)] for i in range(3)])
    E = np.eye(4)
    I = np.eye(3)
    E[:3, :3] = (I + a * Wm) + b * W2
    V = (I + b * Wm) + c * W2
    E[:3, 3] = [(V[i, 0] * xi[0] + V[i, 1] * xi[1]) + V[i, 2] * xi[2] for i in range(3)]
    return E


def step(row, T, damping=DAMPING, dtype=F32):
    """(T after the step in `dtype`, taken): T itself (same bits) where the step is skipped."""
    xi = solve(row, damping)
    if xi is None:
        return T, False
    E = exp_se3(xi)
    T64 = np.asarray(T, np.float64)
    new = T64.copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(4):
                new[i, j] = ((E[i, 0] * T64[0, j] + E[i, 1] * T64[1, j]) + E[i, 2] * T64[2, j]) + E[i, 3] * T64[3, j]
        new = new.astype(dtype)
    if not np.isfinite(new).all():
        return T, False
    return new, True


def fit(depth, flow, K, iK, T0=None, valid=None, iters=4, huber=HUBER, damping=DAMPING, eps=EPS, dtype=F32):
    """(T [N,4,4] in `dtype`, status int32 [N], the row [N,30] at the final T).  dtype=F32: (a), the entry; np.float64: (b)."""
    depth = np.asarray(depth)
    N = depth.shape[0]
    T = np.broadcast_to(np.eye(4, dtype=F32), (N, 4, 4)) if T0 is None else np.asarray(T0)
    T = T.astype(dtype).copy()
    status = np.zeros(N, np.int32)
    for _ in range(iters):
        rows = normal(terms(depth, flow, K, iK, T, valid, huber, eps, dtype))
        for n in range(N):
            if status[n] == 0:
                T[n], taken = step(rows[n], T[n], damping, dtype)
                status[n] = 0 if taken else 1
    return T, status, normal(terms(depth, flow, K, iK, T, valid, huber, eps, dtype))


# ---- the fp32 bound of the module docstring -------------------------------------------------------------------------------------------
def fp32_bound(depth, flow, K, iK, T, valid=None, huber=HUBER, eps=EPS):
    """(bound [N,30] on |normal (a) - normal (b)|, the (b) run) from the operation counts of the module docstring."""
    t = terms(depth, flow, K, iK, T, valid, huber, eps, np.float64)
    N, H, W = t.N, t.H, t.W
    aT, aK, aiK = (np.abs(_mats(m, N, np.float64)) for m in (T, K, iK))
    Kd = _mats(K, N, np.float64)
    at = lambda m, i, j: m[:, i, j][:, None, None]
    x, y = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    d = np.abs(np.asarray(depth, np.float64).reshape(N, H, W))
    with np.errstate(all="ignore"):
        A = [d * (at(aiK, i, 0) * x + at(aiK, i, 1) * y + at(aiK, i, 2)) for i in range(3)]
        Q = [sum(at(aT, i, j) * A[j] for j in range(3)) + at(aT, i, 3) for i in range(3)]
        C = [sum(at(aK, i, j) * Q[j] for j in range(3)) + at(aK, i, 3) for i in range(3)]
        aden = np.abs(t.den)
        dden = 12 * U * C[2] + U * aden
        p, e, tt = [t.px, t.py], [t.ex, t.ey], [t.tx, t.ty]
        Ep = [12 * U * (C[k] + np.abs(p[k]) * C[2]) / aden + 2 * U * np.abs(p[k]) for k in range(2)]
        De = [Ep[k] + U * np.abs(tt[k]) + U * np.abs(e[k]) for k in range(2)]
        dq = [8 * U * Q[i] for i in range(3)]
        DJ = []
        for k in range(2):
            DA = []
            for m in range(3):
                n_ = at(Kd, k, m) - p[k] * at(Kd, 2, m)
                Dn = at(aK, 2, m) * Ep[k] + U * np.abs(p[k] * at(Kd, 2, m)) + U * np.abs(n_)
                a = np.abs(t.J[k][m])
                DA.append(Dn / aden + a * dden / aden + U * a)
            cross = lambda m1, q1, m2, q2, j: (DA[m1] * np.abs(t.q[q1]) + np.abs(t.J[k][m1]) * dq[q1] + U * np.abs(t.J[k][m1] * t.q[q1])
                                               + DA[m2] * np.abs(t.q[q2]) + np.abs(t.J[k][m2]) * dq[q2] + U * np.abs(t.J[k][m2] * t.q[q2])
                                               + U * np.abs(t.J[k][j]))
            DJ.append(DA + [cross(2, 1, 1, 2, 3), cross(0, 2, 2, 0, 4), cross(1, 0, 0, 1, 5)])
        De2 = 2 * (np.abs(e[0]) * De[0] + np.abs(e[1]) * De[1]) + 2 * U * t.e2
        h2 = float(F32(huber)) ** 2
        Dw = np.where(t.e2 + De2 <= h2 * (1 - 2 * U), 0.0, t.w * (De2 / (2 * t.e2) + 2 * U))
        aJ = [[np.abs(v) for v in t.J[k]] for k in range(2)]
        out = []
        for i, j in IDX:
            out.append(t.w * sum(DJ[k][i] * aJ[k][j] + aJ[k][i] * DJ[k][j] for k in range(2))
                       + (3 * U * t.w + Dw) * sum(aJ[k][i] * aJ[k][j] for k in range(2)))
        for i in range(6):
            out.append(t.w * sum(DJ[k][i] * np.abs(e[k]) + aJ[k][i] * De[k] for k in range(2))
                       + (3 * U * t.w + Dw) * sum(aJ[k][i] * np.abs(e[k]) for k in range(2)))
        out += [Dw * t.e2 + t.w * De2 + U * t.w * t.e2, Dw + 0 * t.e2, 0 * t.e2]
        out = np.stack([np.broadcast_to(o, (N, H, W)) for o in out], 1)
        bound = np.where(t.judged[:, None], out, 0.0).reshape(N, SUMS, -1).sum(-1)
    return bound + sum_bound(t), t


# ---- shapes and inputs --------------------------------------------------------------------------------------------------------------------
SIZES, BIG = R.SIZES, R.BIG                    # W in (1, 3, 4, 5, 63, 64, 65, 131) x H in (1, 2, 7), and 131 x 77


def pinhole(H, W, f=20.0):
    """(K, inv_K) fp32 [4,4]: fx = fy = f, the principal point in the middle of the closed image."""
    K = np.array([[f, 0, 0.5 * (W - 1), 0], [0, f, 0.5 * (H - 1), 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64).astype(F32)
    return K, np.linalg.inv(K.astype(np.float64)).astype(F32)


def scene(H, W, N=3, seed=0, noise=0.0, outliers=0.0):
    """Depths in 1 .. 4, fx = fy = 20, a motion of up to 0.1 in translation and 0.03 rad in rotation per image (the issue's
    scene): a namespace depth [N,1,H,W], K, iK [4,4], T [N,4,4] (the truth), flow [N,2,H,W] = the fp64 rigid flow under T rounded to
    fp32, plus noise (pixels) and a share of outliers moved by (3, -2)."""
    rng = np.random.default_rng(9176 * H + 37 * W + 1000003 * seed + 5)
    K, iK = pinhole(H, W)
    depth = rng.uniform(1.0, 4.0, (N, 1, H, W)).astype(F32)
    T = np.stack([R.pose(rng.uniform(-1, 1, 3) * 0.03 / np.sqrt(3), rng.uniform(-1, 1, 3) * 0.1 / np.sqrt(3)) for _ in range(N)])
    flow = R.rigid(depth, T, K, iK, eps=EPS, dtype=np.float64).rigid
    flow = flow + rng.standard_normal(flow.shape) * noise
    if outliers:
        flow = np.where(rng.random((N, 1, H, W)) < outliers, flow + np.array([3.0, -2.0])[None, :, None, None], flow)
    if W == 1:                                 # a closed image one pixel wide: only a target ON the column is judged
        flow[:, 0] = 0.0
    if H == 1:
        flow[:, 1] = 0.0
    return SimpleNamespace(depth=depth, K=K, iK=iK, T=T, flow=flow.astype(F32), eps=EPS, H=H, W=W, N=N)


def start(N, seed=0, scale=0.02):
    """A T0 [N,4,4] fp32 that is not the identity: what the accumulation is tested at."""
    rng = np.random.default_rng(77 + seed)
    return np.stack([R.pose(rng.uniform(-1, 1, 3) * scale, rng.uniform(-1, 1, 3) * scale) for _ in range(N)])


def cases(H, W):
    """[(name, scene, flow, valid or None, huber, T0)] at one shape, N = 3: the input families of the accumulation tests."""
    s = scene(H, W, noise=0.3, outliers=0.1)
    valid = R.mask(H, W, s.N)
    T0 = start(s.N)
    inf = float("inf")
    at_T0 = terms(s.depth, s.flow, s.K, s.iK, T0, None, inf, s.eps)
    # the median residual of the judged pixels: at every shape with two judged pixels, both weight branches occur
    small = float(np.sqrt(np.median(at_T0.e2[at_T0.judged]))) if at_T0.judged.any() else 0.5
    out = [("least squares", s, s.flow, None, inf, T0), ("huber", s, s.flow, None, small, T0),
           ("huber and valid", s, s.flow, valid, small, T0),
           ("at the identity", s, s.flow, valid, 1.0, np.stack([np.eye(4, dtype=F32)] * s.N))]
    bad = scene(H, W, seed=1, noise=0.3)
    bad.depth = R.sprinkle(bad.depth, [0.0, -1.5, np.nan, np.inf], 3 * H + W)
    out.append(("depths of 0, negative, NaN, inf", bad, bad.flow, valid, small, T0))
    out.append(("NaN and inf flow", s, R.sprinkle(s.flow, [np.nan, np.inf, -np.inf], 5 * H + W), None, small, T0))
    out.append(("edge", s, edge_flow(H, W, s.N), None, inf, T0))
    return out


def edge_flow(H, W, N=3):
    """Image 0: every target exactly on (W - 1, H - 1) (judged: the border is closed); image 1: one fp32 step past both (not
    judged, unless the step is lost in x + f); image 2: one fp32 step inside."""
    x, y = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    flow = np.zeros((N, 2, H, W), F32)
    for n, nudge in enumerate((0, 1, -1)):
        tx = np.nextafter(F32(W - 1), F32(np.inf * nudge)) if nudge else F32(W - 1)
        ty = np.nextafter(F32(H - 1), F32(np.inf * nudge)) if nudge else F32(H - 1)
        flow[n, 0], flow[n, 1] = tx - x, ty - y
    return flow


def run(case, dtype=F32):
    name, s, flow, valid, huber, T0 = case
    return terms(s.depth, flow, s.K, s.iK, T0, valid, huber, s.eps, dtype)


# ---- recovery: the reference's own geometry (tests/golden/rigidflow.npz) ----------------------------------------------------------------
# the fixture's scenes on which (b) converges within 6 steps from the identity; 2x3 and 3x4 keep 2 and 4 judged pixels (the others'
# targets leave the image) and are skipped by the fit itself
RECOVERY = [(7, 5), (7, 64), (7, 131), (2, 65), (7, 63), (5, 131), (2, 64), (7, 65)]
RECOVERY_ITERS = 6
RECOVERY_B = 1e-6                 # what "(b) returns the fixture's T" means: max |T_b - T_fixture| (measured: at most 2.7e-7, 2x64;
                                  # the fixture's T and its flow are fp32)
RECOVERY_A_VS_B = 1.3e-7          # measured on the CPU: max |T_a - T_b| over RECOVERY is 1.22e-7 (7x64, 5x131)
RECOVERY_TOL = 4 * RECOVERY_A_VS_B


def golden_scene(rec, H, W):
    """(depth, flow, K, iK, T) of one scene of the fixture: the flow is Project3D's pixel coordinates minus the grid."""
    k = R.golden_key(H, W)
    depth, K, iK, T, pix = (rec[k + "/" + name] for name in ("depth", "K", "inv_K", "T", "pix"))
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    flow = (pix - np.stack([x, y])[None]).astype(F32)
    return depth, flow, K, iK, T


# ---- the moving block -----------------------------------------------------------------------------------------------------------------------
def moving_block(H=24, W=32, top=8, left=12, size=7, shift=5.0, seed=3):
    """The issue's scene: 24x32, depth varying in 1 .. 4, fx = fy = 20, a motion of 0.1 / 0.03 rad, and a size x size block whose
    measured flow is displaced by (+shift, 0).  (scene with N = 1, block mask [H,W] bool)."""
    s = scene(H, W, N=1, seed=seed)
    block = np.zeros((H, W), bool)
    block[top:top + size, left:left + size] = True
    s.flow = s.flow.copy()
    s.flow[0, 0][block] += F32(shift)
    return s, block


def two_rounds(s, rounds=2, iters=4, huber=HUBER, alpha=R.ALPHA, beta=R.BETA, dtype=F32, valid=None):
    """The stream's scheme in NumPy: (T, status, label under the final T, [T after each round])."""
    T, mask, seen = None, valid, []
    for r in range(rounds):
        if r:
            label = R.rigid(s.depth, T.astype(F32), s.K, s.iK, s.flow, valid, alpha, beta, s.eps).label
            mask = (label == 1).astype(np.uint8)
        T, status, _ = fit(s.depth, s.flow, s.K, s.iK, T, mask, iters, huber, DAMPING, s.eps, dtype)
        seen.append(T.copy())
    label = R.rigid(s.depth, T.astype(F32), s.K, s.iK, s.flow, valid, alpha, beta, s.eps).label
    return T, status, label, seen

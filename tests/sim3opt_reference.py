"""Optimizer::OptimizeSim3 restated in NumPy float64, the stand-in for g2o in the Sim3-optimisation tests.

g2o itself cannot be built for these tests: it needs Eigen, which is not available to them.  This file is written from
the sources instead -- Optimizer.cc:3261-3529, OptimizableTypes.h:159-222 (VertexSim3Expmap::oplusImpl, EdgeSim3ProjectXYZ,
EdgeInverseSim3ProjectXYZ), Thirdparty/g2o/g2o/types/sim3.h:50-281, base_binary_edge.hpp:55-205 (constructQuadraticForm
and the NUMERIC linearizeOplus), optimization_algorithm_levenberg.cpp:61-194, robust_kernel_impl.cpp:78, Pinhole.cpp:37-44
-- independently of csrc/vsg_sim3_opt.h: sums over edges are SERIAL in edge order, e12 before e21 of a pair (np.cumsum; an
`order` argument permutes the pairs), sin / cos / exp are libm's.  The dense solve is an LDL^T without pivoting, or
numpy.linalg.solve (solver="numpy"), where Eigen's LDLT pivots.

The quirks it keeps (tests/test_sim3opt_reference.py checks each):
  * the Jacobian is numeric: per column of the Sim3 vertex, central differences with delta = 1e-9 through oplusImpl;
  * _fix_scale zeroes update[6] inside oplusImpl, in the caller's array: column 6 of every Jacobian is exactly 0,
    H(6, 6) = lambda, and computeScale reads the zeroed entry;
  * Sim3::operator* does not normalise the quaternion and the input estimate is taken as it is;
  * the pair set-up is float; with i2 < 0 the second observation is the float NORMALISED coordinate and the octave is
    mnTrackScaleLevel; i2 < 0 && !bAllPoints and P3D2c.z < 0 skip the entry and keep its match;
  * the first check reads the chi2 the LAST computeActiveErrors left (of a rejected trial's state when the last trial
    was rejected), the second computes fresh errors; either chi2 > th2 (double against the widened float) nulls;
  * nCorrespondences - nBad < 10 returns 0 with the matches already nulled and g2oS12 NOT updated;
  * the second optimize() starts again at iteration 0 (lambda re-initialised), 10 iterations after a bad pair, else 5.

For the tolerance measurement (tests/sim3opt_scenes.py) every sin / cos / exp result can be moved by a seeded random
0 or +-1 ulp (`jitter`), the pair order permuted (`order`) and the solver exchanged (`solver`).
"""
import math

import numpy as np

F32 = np.float32
DBL_MAX = float(np.finfo(np.float64).max)
DELTA = 1e-9
NO_EDGE, INLIER, BAD_FIRST, BAD_SECOND, SKIP_Z, SKIP_I2 = 0, 1, 2, 3, 4, 5


class Jitter:
    """Moves a libm result by 0 or +-1 ulp, seeded."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, v):
        k = int(self.rng.integers(-1, 2))
        if k == 0 or not math.isfinite(v):
            return v
        return float(np.nextafter(v, math.inf if k > 0 else -math.inf))


def _same(v):
    return v


def q_rotate(q, v):
    """Eigen's Quaternion::_transformVector; q = x y z w (any norm), v = (..., 3)."""
    x, y, z, w = q
    ux = 2.0 * (y * v[..., 2] - z * v[..., 1])
    uy = 2.0 * (z * v[..., 0] - x * v[..., 2])
    uz = 2.0 * (x * v[..., 1] - y * v[..., 0])
    return np.stack([v[..., 0] + w * ux + (y * uz - z * uy), v[..., 1] + w * uy + (z * ux - x * uz),
                     v[..., 2] + w * uz + (x * uy - y * ux)], -1)


def q_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def q_from_matrix(m):
    """Eigen's Quaterniond(Matrix3d)."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    with np.errstate(all="ignore"):
        if t > 0:
            t = np.sqrt(t + 1.0)
            q[3] = 0.5 * t
            t = 0.5 / t
            q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
            q[i] = 0.5 * t
            t = 0.5 / t
            q[3] = (m[k, j] - m[j, k]) * t
            q[j] = (m[j, i] + m[i, j]) * t
            q[k] = (m[k, i] + m[i, k]) * t
    return q


def sim3(q, t, s):
    return np.array(q, np.float64), np.array(t, np.float64), float(s)


def sim3_exp(u, jit=_same):
    """Sim3(const Vector7d &update) (sim3.h:67-134): update = [omega, upsilon, sigma]."""
    om, up, sigma = u[:3], u[3:6], float(u[6])
    with np.errstate(all="ignore"):
        theta = float(np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]))
        O = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
        # written out: a BLAS product may fuse multiply-adds differently from machine to machine
        O2 = np.array([[(O[i, 0] * O[0, j] + O[i, 1] * O[1, j]) + O[i, 2] * O[2, j] for j in range(3)] for i in range(3)])
        try:
            s = jit(math.exp(sigma))
        except OverflowError:
            s = math.inf
        eye = np.eye(3)
        eps = 0.00001
        if theta < eps:
            sn = cs = None
        else:
            sn, cs = (jit(math.sin(theta)), jit(math.cos(theta))) if math.isfinite(theta) else (math.nan, math.nan)
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B = 1.0 / 2.0, 1.0 / 6.0
                R = eye + O + O2
            else:
                theta2 = theta * theta
                A = (1 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
                R = eye + sn / theta * O + (1 - cs) / (theta * theta) * O2
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = eye + O + O2
            else:
                R = eye + sn / theta * O + (1 - cs) / (theta * theta) * O2
                a, b = s * sn, s * cs
                theta2, sigma2 = theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
        W = A * O + B * O2 + C * eye
        return q_from_matrix(R), np.array([(W[i, 0] * up[0] + W[i, 1] * up[1]) + W[i, 2] * up[2] for i in range(3)]), s


def sim3_map(S, x):
    with np.errstate(all="ignore"):
        return S[2] * q_rotate(S[0], x) + S[1]


def sim3_mul(a, b):
    """operator*: no normalisation."""
    with np.errstate(all="ignore"):
        return q_mul(a[0], b[0]), sim3_map(a, b[1]), a[2] * b[2]


def sim3_inverse(a):
    with np.errstate(all="ignore"):
        qc = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]])
        return qc, q_rotate(qc, (-1.0 / a[2]) * a[1]), 1.0 / a[2]


def oplus(S, u, fix_scale, jit=_same):
    """VertexSim3Expmap::oplusImpl: zeroes u[6] IN PLACE when the scale is fixed."""
    if fix_scale:
        u[6] = 0
    return sim3_mul(sim3_exp(u, jit), S)


def camera_points(Rcw, tcw, Xw):
    """R * P + t in float, as Eigen sums a row: (r0 x + r1 y) + r2 z, then + t."""
    R, t, X = np.asarray(Rcw, F32).reshape(3, 3), np.asarray(tcw, F32), np.asarray(Xw, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


class Problem:
    """The graph of :3313-3450.  kf = dict(Rcw, tcw, fx, fy, cx, cy), kps = dict(x, y, octave) per keyframe."""

    def __init__(self, slots1, slots2, idx2, level2, pos1, pos2, kps1, kps2, kf1, kf2, sig1, sig2, th2, fix_scale,
                 all_points, order=None, jitter=None, solver="ldlt"):
        slots1, slots2, idx2, level2 = (np.asarray(a) for a in (slots1, slots2, idx2, level2))
        n = len(slots1)
        self.state = np.zeros(n, np.uint8)
        cand = np.flatnonzero((slots1 >= 0) & (slots2 >= 0))
        X1c = camera_points(kf1["Rcw"], kf1["tcw"], np.asarray(pos1, F32).reshape(-1, 3)[slots1[cand]])
        X2c = camera_points(kf2["Rcw"], kf2["tcw"], np.asarray(pos2, F32).reshape(-1, 3)[slots2[cand]])
        i2 = idx2[cand]
        skip_i2 = (i2 < 0) & (not all_points)
        skip_z = ~skip_i2 & (X2c[:, 2] < 0)
        self.state[cand[skip_i2]] = SKIP_I2
        self.state[cand[skip_z]] = SKIP_Z
        keep = ~(skip_i2 | skip_z)
        self.feat = cand[keep]
        self.state[self.feat] = INLIER
        E = len(self.feat)
        self.E = E
        i2, X1c, X2c = i2[keep], X1c[keep], X2c[keep]
        self.in_kf2 = i2 >= 0
        self.X1, self.X2 = X1c.astype(np.float64), X2c.astype(np.float64)
        self.obs1 = np.stack([np.asarray(kps1["x"], F32)[self.feat], np.asarray(kps1["y"], F32)[self.feat]], 1).astype(np.float64)
        self.w1 = np.asarray(sig1, F32)[np.asarray(kps1["octave"])[self.feat]].astype(np.float64)
        j = np.where(self.in_kf2, i2, 0)
        with np.errstate(all="ignore"):
            invz = F32(1) / X2c[:, 2]  # float
            nx, ny = X2c[:, 0] * invz, X2c[:, 1] * invz
        k2x, k2y, k2o = np.asarray(kps2["x"], F32), np.asarray(kps2["y"], F32), np.asarray(kps2["octave"])
        if len(k2x) == 0:
            k2x, k2y, k2o = np.zeros(1, F32), np.zeros(1, F32), np.zeros(1, np.int32)
        self.obs2 = np.stack([np.where(self.in_kf2, k2x[j], nx), np.where(self.in_kf2, k2y[j], ny)], 1).astype(np.float64)
        oct2 = np.where(self.in_kf2, k2o[j], level2[self.feat])
        self.w2 = np.asarray(sig2, F32)[oct2].astype(np.float64) if E else np.zeros(0)
        self.cam1 = [float(F32(kf1[k])) for k in ("fx", "fy", "cx", "cy")]
        self.cam2 = [float(F32(kf2[k])) for k in ("fx", "fy", "cx", "cy")]
        self.th2 = float(F32(th2))
        self.delta = float(F32(math.sqrt(float(F32(th2)))))  # const float deltaHuber = sqrt(th2)
        self.fix_scale = bool(fix_scale)
        self.alive = np.ones(E, bool)
        self.chi12, self.chi21 = np.zeros(E), np.zeros(E)  # chi2() as the last computeError left them
        self.robust = True
        self.order = np.arange(E) if order is None else np.asarray(order)
        self.jit = jitter if jitter is not None else _same
        self.solver = solver

    def active(self):
        return self.order[self.alive[self.order]]

    @staticmethod
    def _project(cam, X):
        fx, fy, cx, cy = cam
        with np.errstate(all="ignore"):
            return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)

    def errors(self, S, idx, Sinv=None):
        """computeError of both edges of pairs idx -> e12 (n, 2), e21 (n, 2)."""
        Sinv = sim3_inverse(S) if Sinv is None else Sinv
        e12 = self.obs1[idx] - self._project(self.cam1, sim3_map(S, self.X2[idx]))
        e21 = self.obs2[idx] - self._project(self.cam2, sim3_map(Sinv, self.X1[idx]))
        return e12, e21

    @staticmethod
    def chi2_of(e, w):
        with np.errstate(all="ignore"):
            return e[:, 0] * (w * e[:, 0] + 0.0 * e[:, 1]) + e[:, 1] * (0.0 * e[:, 0] + w * e[:, 1])

    def robustify(self, chi2):
        if not self.robust:
            return chi2, np.ones_like(chi2)
        dsqr = self.delta * self.delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * sq * self.delta - dsqr), np.where(inl, 1.0, self.delta / sq)

    @staticmethod
    def total(a, b):
        """A serial sum over the pairs in the order given, e12's term before e21's."""
        v = np.stack([a, b], 1).reshape((-1,) + a.shape[1:])
        return np.cumsum(v, axis=0)[-1] if len(v) else np.zeros(a.shape[1:])

    def compute_errors(self, S):
        idx = self.active()
        e12, e21 = self.errors(S, idx)
        c12, c21 = self.chi2_of(e12, self.w1[idx]), self.chi2_of(e21, self.w2[idx])
        self.chi12[idx], self.chi21[idx] = c12, c21
        return idx, e12, e21, c12, c21

    def chi(self, S):
        """computeActiveErrors + activeRobustChi2."""
        _, _, _, c12, c21 = self.compute_errors(S)
        with np.errstate(all="ignore"):
            return float(self.total(self.robustify(c12)[0], self.robustify(c21)[0]))

    def build(self, S):
        """computeActiveErrors, activeRobustChi2, linearizeOplus (numeric) and buildSystem -> chi, b (7,), H (7, 7)."""
        idx, e12, e21, c12, c21 = self.compute_errors(S)
        n = len(idx)
        scalar = 1.0 / (2 * DELTA)
        J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
        with np.errstate(all="ignore"):
            for d in range(7):
                add = np.zeros(7)
                add[d] = DELTA
                Sp = oplus(S, add, self.fix_scale, self.jit)
                add[d] = -DELTA
                Sm = oplus(S, add, self.fix_scale, self.jit)
                p12, p21 = self.errors(Sp, idx)
                m12, m21 = self.errors(Sm, idx)
                J12[:, :, d] = scalar * (p12 - m12)
                J21[:, :, d] = scalar * (p21 - m21)
            a12, r12 = self.robustify(c12)
            a21, r21 = self.robustify(c21)
            w1, w2 = self.w1[idx], self.w2[idx]
            # omega_r = -omega * _error, *= rho[1]
            o12 = np.stack([-(w1 * e12[:, 0] + 0.0 * e12[:, 1]) * r12, -(0.0 * e12[:, 0] + w1 * e12[:, 1]) * r12], 1)
            o21 = np.stack([-(w2 * e21[:, 0] + 0.0 * e21[:, 1]) * r21, -(0.0 * e21[:, 0] + w2 * e21[:, 1]) * r21], 1)
            wo12, wo21 = r12 * w1, r21 * w2
            b, H = np.zeros(7), np.zeros((7, 7))
            for a in range(7):
                b[a] = self.total(J12[:, 0, a] * o12[:, 0] + J12[:, 1, a] * o12[:, 1],
                                  J21[:, 0, a] * o21[:, 0] + J21[:, 1, a] * o21[:, 1])
                for k in range(a, 7):
                    H[a, k] = H[k, a] = self.total(
                        (J12[:, 0, a] * wo12) * J12[:, 0, k] + (J12[:, 1, a] * wo12) * J12[:, 1, k],
                        (J21[:, 0, a] * wo21) * J21[:, 0, k] + (J21[:, 1, a] * wo21) * J21[:, 1, k])
            return float(self.total(a12, a21)), b, H, (J12, J21)


def solve7(H, b, lam, solver="ldlt"):
    """LinearSolverDense::solve on H + lambda I -> (ok, x).  ldlt: without pivoting, ok = every pivot positive (a NaN
    pivot passes); numpy: numpy.linalg.solve, ok = positive definite by the same LDL^T's pivots."""
    n = 7
    A = H + lam * np.eye(n)
    L, D, ok = np.eye(n), np.zeros(n), True
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k] * D[k]
            D[j] = d
            if d <= 0.0:
                ok = False
            for i in range(j + 1, n):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k] * D[k]
                L[i, j] = s / d
        if solver == "numpy" and ok and np.isfinite(A).all() and np.isfinite(b).all():
            try:
                return ok, np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                pass
        y, x = np.zeros(n), np.zeros(n)
        for i in range(n):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        for i in range(n - 1, -1, -1):
            s = y[i] / D[i]
            for k in range(i + 1, n):
                s = s - L[k, i] * x[k]
            x[i] = s
    return ok, x


def optimize(P, S, iterations, log=None):
    """SparseOptimizer::optimize(iterations) under OptimizationAlgorithmLevenberg -> the estimate.  log (a dict)
    receives lambda0, trials = [(iteration, lambda used, rho, accepted)], end = qmax | rho0 | nbad | iters, H0, J0 (the
    first build's Hessian and Jacobians)."""
    lam, ni, n_bad = 0.0, 2.0, 0
    trials, end = [], "iters"
    with np.errstate(all="ignore"):
        for it in range(iterations):
            cur, b, H, J = P.build(S)
            ini = cur
            if it == 0:
                md = 0.0
                for j in range(7):
                    d = abs(H[j, j])
                    md = md if d < md else d
                lam, ni, n_bad = 1e-5 * md, 2.0, 0
                if log is not None:
                    log["lambda0"], log["H0"], log["J0"] = lam, H.copy(), J
            rho, qmax = 0.0, 0
            while True:
                ok2, x = solve7(H, b, lam, P.solver)
                cand = oplus(S, x, P.fix_scale, P.jit)  # zeroes x[6] when the scale is fixed; computeScale reads it
                temp = P.chi(cand)
                if not ok2:
                    temp = DBL_MAX
                rho = cur - temp
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                rho /= scale
                good = bool(rho > 0 and math.isfinite(temp))
                trials.append((it, lam, float(rho), good))
                if good:
                    alpha = 1.0 - math.pow(2 * rho - 1, 3)
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = temp
                    S = cand
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                end = "qmax" if qmax == 10 else "rho0"
                break
            if (ini - cur) * 1e3 < ini:
                n_bad += 1
            else:
                n_bad = 0
            if n_bad >= 3:
                end = "nbad"
                break
    if log is not None:
        log["trials"], log["end"] = trials, end
    return S


def optimize_sim3(slots1, slots2, idx2, level2, pos1, pos2, kps1, kps2, kf1, kf2, sig1, sig2, S12, th2, fix_scale,
                  all_points, order=None, jitter=None, solver="ldlt"):
    """-> dict: ret, state (per feature), chi2 {feature: (chi12, chi21) last compared}, S12 = (q, t, s), updated,
    n_correspondences, n_bad, n_in, n_in_kf2, n_out_kf2, more_iterations, log = dict(opt = [per optimisation: lambda0,
    trials, end, H0, J0], first = {feature: (stale12, stale21, fresh12, fresh21)}, compared = [(chi2, th2) ...])."""
    P = Problem(slots1, slots2, idx2, level2, pos1, pos2, kps1, kps2, kf1, kf2, sig1, sig2, th2, fix_scale, all_points,
                order, jitter, solver)
    inp = sim3(*S12)
    out = dict(ret=0, chi2={}, S12=inp, updated=0, n_correspondences=P.E, n_bad=0, n_in=0,
               n_in_kf2=int(P.in_kf2.sum()), n_out_kf2=int((~P.in_kf2).sum()), more_iterations=5,
               log=dict(opt=[], first={}, compared=[]))
    th2 = P.th2
    est = inp
    log = {}
    if P.E > 0:
        est = optimize(P, est, 5, log)
    out["log"]["opt"].append(log)
    # the first check: chi2() of the errors as the last computeActiveErrors left them
    all_idx = np.arange(P.E)
    f12, f21 = P.errors(est, all_idx)
    f12, f21 = P.chi2_of(f12, P.w1), P.chi2_of(f21, P.w2)
    n_bad = 0
    for e in range(P.E):
        f = int(P.feat[e])
        c12, c21 = float(P.chi12[e]), float(P.chi21[e])
        out["log"]["first"][f] = (c12, c21, float(f12[e]), float(f21[e]))
        out["log"]["compared"] += [(c12, th2), (c21, th2)]
        out["chi2"][f] = (c12, c21)
        if c12 > th2 or c21 > th2:
            P.state[f] = BAD_FIRST
            P.alive[e] = False
            n_bad += 1
    P.robust = False
    out["n_bad"] = n_bad
    out["more_iterations"] = 10 if n_bad > 0 else 5
    out["state"] = P.state
    if P.E - n_bad < 10:
        return out
    log = {}
    est = optimize(P, est, out["more_iterations"], log)
    out["log"]["opt"].append(log)
    n_in = 0
    idx = np.flatnonzero(P.alive)
    e12, e21 = P.errors(est, idx)
    c12s, c21s = P.chi2_of(e12, P.w1[idx]), P.chi2_of(e21, P.w2[idx])
    for e, c12, c21 in zip(idx, c12s, c21s):
        f = int(P.feat[e])
        out["chi2"][f] = (float(c12), float(c21))
        out["log"]["compared"] += [(float(c12), th2), (float(c21), th2)]
        if c12 > th2 or c21 > th2:
            P.state[f] = BAD_SECOND
        else:
            n_in += 1
    out["n_in"], out["ret"], out["S12"], out["updated"] = n_in, n_in, est, 1
    return out


def min_threshold_margin(result):
    """The smallest relative distance of a compared chi2 from th2 over a run (inf when nothing compared)."""
    m = math.inf
    for c, th in result["log"]["compared"]:
        if np.isfinite(c):
            m = min(m, abs(float(c) - float(th)) / float(th))
    return m

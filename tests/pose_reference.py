"""Optimizer::PoseOptimization(Frame *) restated in NumPy float64, the stand-in for g2o in the pose tests.

g2o itself cannot be built for these tests: it needs Eigen, which is not available to them.  This file is written from
the sources instead -- Optimizer.cc:1063-1452 (the !mpCamera2 branches), optimization_algorithm_levenberg.cpp:61-194,
sparse_optimizer.cpp:399-, base_unary_edge.hpp:43-72, robust_kernel_impl.cpp:78, OptimizableTypes.cpp:47-62,
Pinhole.cpp:37-44 / :78-89, types_six_dof_expmap.cpp:365-437, se3quat.h and linear_solver_dense.h -- independently of
csrc/vsg_pose_opt.h: sums over edges are SERIAL in edge order (np.cumsum; an `order` argument permutes them), sin / cos
/ pow are libm's.  The dense solve is an LDL^T without pivoting, where Eigen's LDLT pivots: on these well-conditioned
6x6 systems the two agree to rounding, which the measured tolerance of pose_scenes.py absorbs.

The quirks it keeps (tests/test_pose_reference.py checks each):
  * every round restarts from the frame's pose; lambda, ni and nBad restart with every optimize();
  * an inlier edge's chi2 at classification is the one the LAST computeActiveErrors left, i.e. of a rejected trial's
    state when the last trial was rejected; an outlier edge's is recomputed at the estimate;
  * chi2 is narrowed to float and compared with 5.991f / 7.815f by `>`; the Huber deltas are floats; the kernel goes
    in round 2's classification; comparisons are written as the reference has them, so NaN passes;
  * fewer than 3 edges return 0 with the flags cleared; fewer than 10 edges end the loop after one round;
  * features removed by the host's plane step between round 2's optimize and its classification stay flagged and are
    counted in nBad in rounds 2 and 3.
"""
import math

import numpy as np

F32 = np.float32
DELTA = (float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815))))  # deltaMono, deltaStereo
TH = (F32(5.991), F32(7.815))
DBL_MAX = float(np.finfo(np.float64).max)


def q_rotate(q, v):
    """Eigen's Quaternion::_transformVector; q = x y z w, v = (..., 3)."""
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


def q_normalize(q):
    q = np.array(q, np.float64)
    if q[3] < 0:
        q = q * -1
    with np.errstate(all="ignore"):
        return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def q_from_matrix(m):
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
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
        with np.errstate(all="ignore"):
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
            q[i] = 0.5 * t
            t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def q_to_matrix(q):
    return q_rotate(q, np.eye(3)).T


def est_from_pose(q, t):
    return q_normalize(np.asarray(q, F32).astype(np.float64)), np.asarray(t, F32).astype(np.float64)


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:239-269): update = [omega, upsilon] -> (q, t)."""
    om, up = u[:3], u[3:]
    with np.errstate(all="ignore"):
        th = float(np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]))
        O = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
        O2 = O @ O
        if th < 0.00001:
            R = np.eye(3) + O + O2
            V = R
        else:
            s, c = (math.sin(th), math.cos(th)) if math.isfinite(th) else (math.nan, math.nan)
            R = np.eye(3) + s / th * O + (1 - c) / (th * th) * O2
            V = np.eye(3) + (1 - c) / (th * th) * O + (th - s) / math.pow(th, 3) * O2
        return q_normalize(q_from_matrix(R)), V @ up


def oplus(est, u):
    """setEstimate(SE3Quat::exp(update) * estimate())."""
    with np.errstate(all="ignore"):
        q, t = se3_exp(u)
        return q_normalize(q_mul(q, est[0])), t + q_rotate(q, est[1])


class Problem:
    def __init__(self, feat_slots, world_pos, kps_xy, octave, u_right, cam, inv_level_sigma2, order=None):
        feat_slots = np.asarray(feat_slots)
        self.feat = np.flatnonzero(feat_slots >= 0)
        E = len(self.feat)
        self.E = E
        self.X = np.asarray(world_pos, F32)[feat_slots[self.feat]].astype(np.float64).reshape(E, 3)
        ur = np.asarray(u_right, F32)[self.feat] if u_right is not None else np.full(E, -1, F32)
        self.stereo = ~(ur < 0)
        xy = np.asarray(kps_xy, F32)[self.feat].astype(np.float64).reshape(E, 2)
        self.obs = np.concatenate([xy, np.where(self.stereo, ur.astype(np.float64), 0.0)[:, None]], 1)
        self.w = np.asarray(inv_level_sigma2, F32)[np.asarray(octave)[self.feat]].astype(np.float64)
        self.cam = [float(F32(c)) for c in cam]  # fx fy cx cy bf
        self.outlier = np.zeros(E, bool)
        self.removed = np.zeros(E, bool)
        self.gone = np.zeros(E, bool)
        self.chi2 = np.zeros(E)      # each edge's chi2() as its last computeError left it
        self.robust = True
        self.order = np.arange(E) if order is None else np.asarray(order)

    def active(self):
        return self.order[~(self.outlier | self.removed)[self.order]]

    def errors(self, est, idx):
        """computeError + chi2() of edges idx at est -> (e (n, 3), Xc (n, 3), chi2 (n,))."""
        fx, fy, cx, cy, bf = self.cam
        with np.errstate(all="ignore"):
            Xc = q_rotate(est[0], self.X[idx]) + est[1]
            st, obs, w = self.stereo[idx], self.obs[idx], self.w[idx]
            x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
            m0 = obs[:, 0] - (fx * x / z + cx)
            m1 = obs[:, 1] - (fy * y / z + cy)
            invz = (1.0 / z).astype(F32).astype(np.float64)  # const float invz = 1.0f / trans_xyz[2]
            su = x * invz * fx + cx
            s0, s1, s2 = obs[:, 0] - su, obs[:, 1] - (y * invz * fy + cy), obs[:, 2] - (su - bf * invz)
            e = np.stack([np.where(st, s0, m0), np.where(st, s1, m1), np.where(st, s2, 0.0)], 1)
            # _error.dot(information() * _error) with the information matrix's zeros multiplied out
            c2 = e[:, 0] * (w * e[:, 0] + 0.0 * e[:, 1]) + e[:, 1] * (0.0 * e[:, 0] + w * e[:, 1])
            c3 = (e[:, 0] * ((w * e[:, 0] + 0.0 * e[:, 1]) + 0.0 * e[:, 2]) +
                  e[:, 1] * ((0.0 * e[:, 0] + w * e[:, 1]) + 0.0 * e[:, 2])) + e[:, 2] * ((0.0 * e[:, 0] + 0.0 * e[:, 1]) + w * e[:, 2])
            return e, Xc, np.where(st, c3, c2)

    def jacobians(self, Xc, idx):
        fx, fy, cx, cy, bf = self.cam
        n = len(idx)
        with np.errstate(all="ignore"):
            x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
            zero, one = np.zeros(n), np.ones(n)
            P = [[fx / z, zero, -fx * x / (z * z)], [zero, fy / z, -fy * y / (z * z)]]
            D = [[zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero], [y, -x, zero, zero, zero, one]]
            Jm = np.zeros((n, 3, 6))
            for i in range(2):
                for j in range(6):
                    Jm[:, i, j] = (-P[i][0] * D[0][j] + -P[i][1] * D[1][j]) + -P[i][2] * D[2][j]
            invz = 1.0 / z
            invz_2 = invz * invz
            Js = np.zeros((n, 3, 6))
            Js[:, 0, 0] = x * y * invz_2 * fx
            Js[:, 0, 1] = -(1 + (x * x * invz_2)) * fx
            Js[:, 0, 2] = y * invz * fx
            Js[:, 0, 3] = -invz * fx
            Js[:, 0, 5] = x * invz_2 * fx
            Js[:, 1, 0] = (1 + y * y * invz_2) * fy
            Js[:, 1, 1] = -x * y * invz_2 * fy
            Js[:, 1, 2] = -x * invz * fy
            Js[:, 1, 4] = -invz * fy
            Js[:, 1, 5] = y * invz_2 * fy
            Js[:, 2, 0] = Js[:, 0, 0] - bf * y * invz_2
            Js[:, 2, 1] = Js[:, 0, 1] + bf * x * invz_2
            Js[:, 2, 2] = Js[:, 0, 2]
            Js[:, 2, 3] = Js[:, 0, 3]
            Js[:, 2, 5] = Js[:, 0, 5] - bf * invz_2
            return np.where(self.stereo[idx][:, None, None], Js, Jm)

    def robustify(self, chi2, idx):
        """RobustKernelHuber::robustify -> rho0, rho1 (or the identity once the kernel is gone)."""
        if not self.robust:
            return chi2, np.ones_like(chi2)
        delta = np.where(self.stereo[idx], DELTA[1], DELTA[0])
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)

    @staticmethod
    def total(v):
        """A serial sum in the order given (np.add.reduce would sum pairwise)."""
        return np.cumsum(v, axis=0)[-1] if len(v) else np.zeros(v.shape[1:])

    def chi(self, est):
        """computeActiveErrors + activeRobustChi2."""
        idx = self.active()
        _, _, c = self.errors(est, idx)
        self.chi2[idx] = c
        with np.errstate(all="ignore"):
            return float(self.total(self.robustify(c, idx)[0]))

    def build(self, est):
        """computeActiveErrors, activeRobustChi2 and buildSystem -> chi, b (6,), H (6, 6)."""
        idx = self.active()
        e, Xc, c = self.errors(est, idx)
        self.chi2[idx] = c
        with np.errstate(all="ignore"):
            rho0, rho1 = self.robustify(c, idx)
            J = self.jacobians(Xc, idx)
            st, w = self.stereo[idx], self.w[idx]
            wo = rho1 * w
            b, H = np.zeros(6), np.zeros((6, 6))
            for a in range(6):
                t2 = (0.0 + ((rho1 * J[:, 0, a]) * w) * e[:, 0]) + ((rho1 * J[:, 1, a]) * w) * e[:, 1]
                t3 = t2 + ((rho1 * J[:, 2, a]) * w) * e[:, 2]
                b[a] = -self.total(np.where(st, t3, t2))
                for k in range(a, 6):
                    s2 = (0.0 + (J[:, 0, a] * wo) * J[:, 0, k]) + (J[:, 1, a] * wo) * J[:, 1, k]
                    s3 = s2 + (J[:, 2, a] * wo) * J[:, 2, k]
                    H[a, k] = H[k, a] = self.total(np.where(st, s3, s2))
            return float(self.total(rho0)), b, H


def solve6(H, b, lam):
    """LinearSolverDense::solve on H + lambda I -> (ok, x): LDL^T, ok = every pivot positive (a NaN pivot passes)."""
    A = H + lam * np.eye(6)
    L, D, ok = np.eye(6), np.zeros(6), True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k] * D[k]
            D[j] = d
            if d <= 0.0:
                ok = False
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k] * D[k]
                L[i, j] = s / d
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        for i in range(5, -1, -1):
            s = y[i] / D[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s
    return ok, x


def optimize(P, est, log=None):
    """SparseOptimizer::optimize(10) under OptimizationAlgorithmLevenberg -> the estimate.  log (a dict) receives
    lambda0, trials = [(iteration, lambda used, rho, accepted)], end = qmax | rho0 | nbad | iters."""
    lam, ni, n_bad = 0.0, 2.0, 0
    trials, end = [], "iters"
    with np.errstate(all="ignore"):
        for it in range(10):
            cur, b, H = P.build(est)
            ini = cur
            if it == 0:
                md = 0.0
                for j in range(6):
                    d = abs(H[j, j])
                    md = md if d < md else d  # std::max(fabs(v->hessian(j, j)), maxDiagonal)
                lam, ni, n_bad = 1e-5 * md, 2.0, 0
                if log is not None:
                    log["lambda0"] = lam
            rho, qmax = 0.0, 0
            while True:
                ok2, x = solve6(H, b, lam)
                cand = oplus(est, x)
                temp = P.chi(cand)
                if not ok2:
                    temp = DBL_MAX
                rho = cur - temp
                scale = 0.0
                for j in range(6):
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
                    est = cand
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
    return est


def pose_optimization(feat_slots, world_pos, kps_xy, octave, u_right, pose_q, pose_t, cam, inv_level_sigma2,
                      hold_round=-1, removed=None, order=None):
    """-> dict: ret, outlier {feature: flag}, chi2 {feature: float32}, q, t, n_initial, n_bad, rounds_run, held,
    held_q / held_t (the estimate after round 2's optimize), log = [per round: lambda0, trials, end, stale_differs, stale_differs_float, fresh, compared =
    [(feature, chi2 float, threshold)]]."""
    P = Problem(feat_slots, world_pos, kps_xy, octave, u_right, cam, inv_level_sigma2, order)
    inp = est_from_pose(pose_q, pose_t)
    out = dict(ret=0, outlier={int(f): 0 for f in P.feat}, chi2={}, q=inp[0], t=inp[1], n_initial=P.E, n_bad=0,
               rounds_run=0, held=0, log=[])
    if P.E < 3:
        return out
    est, n_bad, edges_left = inp, 0, P.E
    for it in range(4):
        log = {}
        est = optimize(P, inp, log)  # Tcw = pFrame->GetPose(): the INPUT pose in every round
        if it == 2 and hold_round == 2:
            out["held"], out["held_q"], out["held_t"] = 1, est[0].copy(), est[1].copy()
            if removed is not None:
                rem = np.asarray(removed)[P.feat] != 0
                P.removed |= rem
                P.outlier |= rem
        n_bad, compared = 0, []
        if it == 2:
            P.robust = False
        # how many inlier edges carry an error that is NOT the one at the estimate (the last trial was rejected)
        inl = np.flatnonzero(~(P.outlier | P.removed))
        fresh = P.errors(est, inl)[2]
        log["stale_differs"] = int((fresh != P.chi2[inl]).sum())
        with np.errstate(all="ignore"):
            ff, sf = fresh.astype(F32), P.chi2[inl].astype(F32)
        fin = np.isfinite(ff) & np.isfinite(sf)
        log["stale_differs_float"] = int((fin & (ff != sf)).sum())     # on finite values only: NaN != NaN says nothing
        log["fresh"] = {int(P.feat[e]): c for e, c in zip(inl, ff)}  # what a recomputing implementation would compare
        for e in range(P.E):
            if P.outlier[e]:
                if P.removed[e]:
                    if not P.gone[e]:
                        P.gone[e] = True
                        edges_left -= 1
                    n_bad += 1
                    continue
                P.chi2[e] = P.errors(est, np.array([e]))[2][0]
            with np.errstate(all="ignore"):
                c = F32(P.chi2[e])
            th = TH[1] if P.stereo[e] else TH[0]
            compared.append((int(P.feat[e]), c, th))
            out["chi2"][int(P.feat[e])] = c
            if c > th:
                P.outlier[e] = True
                n_bad += 1
            else:
                P.outlier[e] = False
        log["compared"] = compared
        out["log"].append(log)
        out["rounds_run"] = it + 1
        if edges_left < 10:
            break
    out["outlier"] = {int(f): int(o) for f, o in zip(P.feat, P.outlier)}
    out["q"], out["t"], out["n_bad"], out["ret"] = est[0], est[1], n_bad, P.E - n_bad
    return out


def min_threshold_margin(result):
    """The smallest relative distance of a compared chi2 from its threshold over a run (inf when nothing compared)."""
    m = math.inf
    for log in result["log"]:
        for _, c, th in log["compared"]:
            if np.isfinite(c):
                m = min(m, abs(float(c) - float(th)) / float(th))
    return m

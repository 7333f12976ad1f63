"""The visual part of Optimizer::LocalBundleAdjustment restated in NumPy float64, the stand-in for g2o in the local-BA tests.

g2o cannot be built for these tests (it needs Eigen).  This file is written from the sources instead -- Optimizer.cc:1454-2454
(keyframe and point vertices, EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ edges, the classification and the recovery),
OptimizableTypes.cpp:135-161, types_six_dof_expmap.cpp:202-297, base_binary_edge.hpp:55-116, robust_kernel_impl.cpp:78,
block_solver.hpp:354-605 and optimization_algorithm_levenberg.cpp:61-199 -- independently of csrc/vsg_local_ba.h: every sum
over edges is SERIAL in edge order (np.add.at and np.cumsum; an `order` argument permutes the edges), sin / cos / pow are
libm's, the point blocks are inverted by numpy, the reduced system is dense and solved by an LDL^T without pivoting in the
keyframes' order (the reference: SimplicialLDLT behind an AMD ordering; equal to rounding on a positive-definite system).
The quaternion and SE3 helpers are those of pose_reference.py.

The quirks it keeps (tests/test_lba_reference.py checks each on a directed scene):
  * the chi2 compared at the classification is the one the LAST computeActiveErrors left: of a rejected trial's state when
    the last trial was rejected, although pop() restored the estimates; isDepthPositive is evaluated on the restored ones;
  * the comparisons are `> 5.991`, `> 7.815` in double; the Huber deltas are floats;
  * a non-positive pivot makes tempChi DBL_MAX; qmax == 10 or rho == 0 terminates; three iterations in a row that gain
    less than a thousandth stop the run;
  * a keyframe without edges and a point without observations are no vertices; a fixed keyframe's edges fill the point's
    blocks alone.
"""
import numpy as np

from pose_reference import DBL_MAX, DELTA, F32, est_from_pose, oplus, q_rotate

TH = (5.991, 7.815)
STOP_ITERATIONS, STOP_TERMINATE, STOP_BAD, STOP_FLAG = 0, 1, 2, 3


def rot_matrices(Q):
    """Eigen's toRotationMatrix for quaternions (n, 4) x y z w -> (n, 3, 3)."""
    x, y, z, w = Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.empty((len(Q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 - (tyy + tzz), txy - twz, txz + twy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = txy + twz, 1.0 - (txx + tzz), tyz - twx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = txz - twy, tyz + twx, 1.0 - (txx + tyy)
    return R


def ldlt_solve(A, b):
    """A x = b by LDL^T without pivoting -> (ok, x); ok = every pivot positive (a NaN pivot passes)."""
    n = len(b)
    L, D, ok = np.eye(n), np.zeros(n), True
    with np.errstate(all="ignore"):
        for j in range(n):
            v = L[j, :j] * D[:j]
            d = A[j, j] - L[j, :j] @ v
            D[j] = d
            if d <= 0.0:
                ok = False
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ v) / d
        y = np.zeros(n)
        for i in range(n):
            y[i] = b[i] - L[i, :i] @ y[:i]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = y[i] / D[i] - L[i + 1:, i] @ x[i + 1:]
    return ok, x


class Graph:
    def __init__(self, s, order=None):
        self.K, self.P = len(s["kfs"]), len(s["slots"])
        off = np.asarray(s["obs_off"])
        self.E = E = int(off[-1])
        self.kf = np.asarray(s["obs_kf"], np.int64)[:E]
        idx = np.asarray(s["obs_idx"], np.int64)[:E]
        self.pt = np.repeat(np.arange(self.P), np.diff(off))
        self.fixed = np.asarray(s["fixed"]).astype(bool)
        x = np.array([s["kfs"][k]["x"][i] for k, i in zip(self.kf, idx)], F32)
        y = np.array([s["kfs"][k]["y"][i] for k, i in zip(self.kf, idx)], F32)
        oc = np.array([s["kfs"][k]["octave"][i] for k, i in zip(self.kf, idx)], np.int64)
        ur = np.array([-1.0 if s["kfs"][k]["ur"] is None else s["kfs"][k]["ur"][i] for k, i in zip(self.kf, idx)], F32)
        self.stereo = ur >= 0
        self.obs = np.stack([x.astype(np.float64), y.astype(np.float64), np.where(self.stereo, ur.astype(np.float64), 0.0)], 1)
        self.w = np.asarray(s["sig"], F32)[oc].astype(np.float64)
        self.cam = np.asarray(s["cam"], F32).astype(np.float64)[self.kf]  # per edge: fx fy cx cy bf
        has = np.bincount(self.kf, minlength=self.K) > 0
        self.opt_kf = np.flatnonzero(~self.fixed & has)
        self.Ko = len(self.opt_kf)
        opt_of = np.full(self.K, -1)
        opt_of[self.opt_kf] = np.arange(self.Ko)
        self.eo = opt_of[self.kf]  # per edge: index among the optimised keyframes, -1 fixed
        self.vertex_pt = np.diff(off) > 0
        self.order = np.arange(E) if order is None else np.asarray(order)
        self.est = [est_from_pose(T[:4], T[4:]) for T in np.asarray(s["Tcw"], F32)]
        self.X = np.asarray(s["store_pos"], F32)[np.asarray(s["slots"])].astype(np.float64).reshape(self.P, 3)
        self.chi2 = np.zeros(E)
        # ordered pairs (a, b) of edges of one point, both on optimised keyframes
        pa, pb = [], []
        for p in range(self.P):
            es = [e for e in range(off[p], off[p + 1]) if self.eo[e] >= 0]
            for a in es:
                for b in es:
                    pa.append(a), pb.append(b)
        self.pa, self.pb = np.array(pa, np.int64), np.array(pb, np.int64)

    def camera_points(self, est, X):
        Q = np.array([est[k][0] for k in range(self.K)])[self.kf]
        t = np.array([est[k][1] for k in range(self.K)])[self.kf]
        with np.errstate(all="ignore"):
            return q_rotate(Q.T, X[self.pt]) + t, Q

    def errors(self, est, X):
        """computeError + chi2() of every edge -> e (E, 3), Xc, Q, chi2."""
        fx, fy, cx, cy, bf = self.cam.T
        Xc, Q = self.camera_points(est, X)
        with np.errstate(all="ignore"):
            x, y, z = Xc.T
            m0, m1 = self.obs[:, 0] - (fx * x / z + cx), self.obs[:, 1] - (fy * y / z + cy)
            invz = (1.0 / z).astype(F32).astype(np.float64)
            su = x * invz * fx + cx
            s0, s1, s2 = self.obs[:, 0] - su, self.obs[:, 1] - (y * invz * fy + cy), self.obs[:, 2] - (su - bf * invz)
            st = self.stereo
            e = np.stack([np.where(st, s0, m0), np.where(st, s1, m1), np.where(st, s2, 0.0)], 1)
            chi2 = self.w * (e * e).sum(1)
        return e, Xc, Q, chi2

    def robustify(self, chi2):
        delta = np.where(self.stereo, DELTA[1], DELTA[0])
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)

    def serial(self, v):
        v = v[self.order]
        return float(np.cumsum(v)[-1]) if len(v) else 0.0

    def chi(self, est, X):
        _, _, _, c = self.errors(est, X)
        self.chi2 = c
        with np.errstate(all="ignore"):
            return self.serial(self.robustify(c)[0])

    def jacobians(self, Xc, Q):
        fx, fy, cx, cy, bf = self.cam.T
        E = self.E
        R = rot_matrices(Q)
        with np.errstate(all="ignore"):
            x, y, z = Xc.T
            z_2 = z * z
            zero, one = np.zeros(E), np.ones(E)
            Pn = np.zeros((E, 3, 3))  # -projectJac, third row empty
            Pn[:, 0, 0], Pn[:, 0, 2], Pn[:, 1, 1], Pn[:, 1, 2] = -(fx / z), fx * x / z_2, -(fy / z), fy * y / z_2
            D = np.stack([np.stack(r, 1) for r in ([zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero],
                                                   [y, -x, zero, zero, zero, one])], 1)
            Am, Bm = Pn @ R, Pn @ D
            As, Bs = np.zeros((E, 3, 3)), np.zeros((E, 3, 6))
            for j in range(3):
                As[:, 0, j] = -fx * R[:, 0, j] / z + fx * x * R[:, 2, j] / z_2
                As[:, 1, j] = -fy * R[:, 1, j] / z + fy * y * R[:, 2, j] / z_2
                As[:, 2, j] = As[:, 0, j] - bf * R[:, 2, j] / z_2
            Bs[:, 0, 0], Bs[:, 0, 1], Bs[:, 0, 2] = x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx
            Bs[:, 0, 3], Bs[:, 0, 5] = -1. / z * fx, x / z_2 * fx
            Bs[:, 1, 0], Bs[:, 1, 1], Bs[:, 1, 2] = (1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy
            Bs[:, 1, 4], Bs[:, 1, 5] = -1. / z * fy, y / z_2 * fy
            Bs[:, 2, 0], Bs[:, 2, 1] = Bs[:, 0, 0] - bf * y / z_2, Bs[:, 0, 1] + bf * x / z_2
            Bs[:, 2, 2], Bs[:, 2, 3], Bs[:, 2, 5] = Bs[:, 0, 2], Bs[:, 0, 3], Bs[:, 0, 5] - bf / z_2
        st = self.stereo[:, None, None]
        return np.where(st, As, Am), np.where(st, Bs, Bm)

    def build(self, est, X):
        """computeActiveErrors, activeRobustChi2, buildSystem."""
        e, Xc, Q, c = self.errors(est, X)
        self.chi2 = c
        with np.errstate(all="ignore"):
            rho0, rho1 = self.robustify(c)
            A, B = self.jacobians(Xc, Q)
            wo = rho1 * self.w
            omega_r = -(self.w[:, None] * e) * rho1[:, None]
            At, Bt = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
            o, eo = self.order, self.eo
            self.Hll, self.bl = np.zeros((self.P, 3, 3)), np.zeros((self.P, 3))
            np.add.at(self.Hll, self.pt[o], ((At * wo[:, None, None]) @ A)[o])
            np.add.at(self.bl, self.pt[o], (At @ omega_r[:, :, None])[o, :, 0])
            oo = o[eo[o] >= 0]
            self.Hpp, self.bp = np.zeros((self.Ko, 6, 6)), np.zeros((self.Ko, 6))
            np.add.at(self.Hpp, eo[oo], ((Bt * wo[:, None, None]) @ B)[oo])
            np.add.at(self.bp, eo[oo], (Bt @ omega_r[:, :, None])[oo, :, 0])
            self.Hpl = (Bt * wo[:, None, None]) @ A  # (E, 6, 3); rows of fixed keyframes unused
            return self.serial(rho0)

    def lambda_init(self):
        d = np.concatenate([np.abs(np.einsum("kii->ki", self.Hpp)).ravel(),
                            np.abs(np.einsum("pii->pi", self.Hll))[self.vertex_pt].ravel()])
        return 1e-5 * float(np.max(d)) if len(d) else 0.0

    def solve(self, lam):
        """setLambda, the Schur complement, the reduced solve, the back-substitution -> ok2, xp (Ko, 6), xl (P, 3)."""
        Ko, eo = self.Ko, self.eo
        with np.errstate(all="ignore"):
            Hll = self.Hll + lam * np.eye(3)
            Hll[~self.vertex_pt] = np.eye(3)
            Dinv = np.linalg.inv(Hll)
            W = self.Hpl @ Dinv[self.pt]  # B Dinv per edge
            Hs = np.zeros((Ko, Ko, 6, 6))
            Hs[np.arange(Ko), np.arange(Ko)] = self.Hpp + lam * np.eye(6)
            if len(self.pa):
                np.subtract.at(Hs, (eo[self.pa], eo[self.pb]), W[self.pa] @ self.Hpl[self.pb].transpose(0, 2, 1))
            bs = self.bp.copy()
            oo = self.order[eo[self.order] >= 0]
            np.subtract.at(bs, eo[oo], (W @ self.bl[self.pt][:, :, None])[oo, :, 0])
            ok, xp = ldlt_solve(Hs.transpose(0, 2, 1, 3).reshape(6 * Ko, 6 * Ko), bs.reshape(-1))
            xp = xp.reshape(Ko, 6)
            r = self.bl.copy()
            np.subtract.at(r, self.pt[oo], (self.Hpl.transpose(0, 2, 1)[oo] @ xp[eo[oo]][:, :, None])[:, :, 0])
            xl = (Dinv @ r[:, :, None])[:, :, 0]
            xl[~self.vertex_pt] = 0.0
        return ok, xp, xl


def local_ba(s, order=None, stop_flag=False):
    """-> dict(ran, kf_out (K, 7) f64, pos_out (P, 3) f32, erase, chi2, the counters of vsg_local_ba_result, and `trace`:
    per iteration the list of (rho, accepted, ok2) of its trials)."""
    K, P = len(s["kfs"]), len(s["slots"])
    Tin = np.asarray(s["Tcw"], F32).reshape(K, 7)
    pos_in = np.asarray(s["store_pos"], F32)[np.asarray(s["slots"], np.int64)].reshape(P, 3)
    fixed = np.asarray(s["fixed"]).astype(bool)
    E = int(np.asarray(s["obs_off"])[-1]) if P else 0
    out = dict(ran=0, kf_out=Tin.astype(np.float64), pos_out=pos_in.copy(), erase=np.zeros(E, np.uint8), chi2=np.zeros(E),
               n_opt_kf=int((~fixed).sum()) if P else 0, n_fixed_kf=int(fixed.sum()) if P else 0, n_points=P, n_edges=E, trace=[])
    if P == 0 or not fixed.any() or E == 0 or stop_flag:  # :1734, :2277, :2283
        return out
    g = Graph(s, order)
    est, X = list(g.est), g.X.copy()
    lam = ni = 0.0
    n_bad = its = trials = 0
    stop, chi_initial, current = STOP_ITERATIONS, 0.0, 0.0
    with np.errstate(all="ignore"):
        for it in range(s["iterations"]):
            current = g.build(est, X)
            ini = current
            if it == 0:
                lam, ni, n_bad, chi_initial = g.lambda_init(), 2.0, 0, current
            rho, qmax, tr = 0.0, 0, []
            while True:
                ok2, xp, xl = g.solve(lam)
                cand = list(est)
                for i, k in enumerate(g.opt_kf):
                    cand[k] = oplus(est[k], xp[i])
                Xc = X + xl
                temp = g.chi(cand, Xc)
                if not ok2:
                    temp = DBL_MAX
                xs = np.concatenate([xp.ravel(), xl[g.vertex_pt].ravel()])
                bsv = np.concatenate([g.bp.ravel(), g.bl[g.vertex_pt].ravel()])
                sc = xs * (lam * xs + bsv)
                scale = (float(np.cumsum(sc)[-1]) if len(sc) else 0.0) + 1e-3
                rho = (current - temp) / scale
                good = bool(rho > 0 and np.isfinite(temp))
                if good:
                    alpha = min(1. - float(np.float64(2 * rho - 1) ** 3), 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni, current, est, X = 2.0, temp, cand, Xc
                else:
                    lam *= ni
                    ni *= 2
                tr.append((float(rho), good, bool(ok2)))
                qmax += 1
                trials += 1
                if not (rho < 0 and qmax < 10):
                    break
            out["trace"].append(tr)
            its += 1
            if qmax == 10 or rho == 0:
                stop = STOP_TERMINATE
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                stop = STOP_BAD
                break
        Xcam, _ = g.camera_points(est, X)
        depth_positive = Xcam[:, 2] > 0.0
        th = np.where(g.stereo, TH[1], TH[0])
        out["erase"] = ((g.chi2 > th) | ~depth_positive).astype(np.uint8)
        out["depth_positive"] = depth_positive
        _, _, _, out["chi2_fresh"] = g.errors(est, X)
    out["chi2"] = g.chi2.copy()
    for k in g.opt_kf:
        out["kf_out"][k] = np.concatenate(est[k])
    out["pos_out"][g.vertex_pt] = X[g.vertex_pt].astype(F32)
    out.update(ran=1, n_mono=int((~g.stereo).sum()), n_stereo=int(g.stereo.sum()), n_erase=int(out["erase"].sum()),
               iterations_run=its, trials_run=trials, stop_reason=stop, **{"lambda": lam}, chi2_initial=chi_initial,
               chi2_final=current, th=th)
    return out

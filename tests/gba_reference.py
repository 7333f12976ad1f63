"""The visual part of Optimizer::BundleAdjustment (Optimizer.cc:60-287, :500-610, behind GlobalBundleAdjustemnt :45-58)
restated in NumPy float64, the stand-in for g2o in the global-BA tests.

It is written from the sources, independently of csrc/vsg_global_ba.h.  The graph is the local BA's (VertexSE3Expmap,
VertexSBAPointXYZ, EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ, BlockSolverX behind OptimizationAlgorithmLevenberg), so the
edges, the Jacobians, buildSystem, the Schur complement and the dense LDL^T come from lba_reference.Graph unchanged.  What
this routine has of its own is restated here:
  * the robust kernel is set only `if (bRobust)` (:189, :221) and its deltas are the floats sqrt(5.99) and sqrt(7.815)
    (:133-134) -- 5.99, where LocalBundleAdjustment has 5.991; without a kernel rho = chi2 and the weight is 1;
  * a keyframe is fixed when mnId == GetInitKFid() (:126) and NO fixed keyframe is no reason to return;
  * a point without an edge is removed and marked vbNotIncludedMP (:278-286);
  * optimize(nIterations) (:500-503) and the write-back (:505-610): vSE3->estimate() per keyframe, the float position per
    included point; nothing is classified, and e->chi2() is what the LAST computeActiveErrors left.
"""
import math

import numpy as np

import lba_reference as lr
from pose_reference import DBL_MAX, F32, oplus

DELTA = (float(F32(math.sqrt(5.99))), float(F32(math.sqrt(7.815))))  # thHuber2D, thHuber3D
STOP_ITERATIONS, STOP_TERMINATE, STOP_BAD, STOP_FLAG = 0, 1, 2, 3


class Graph(lr.Graph):
    def __init__(self, s, order=None):
        super().__init__(s, order)
        self.robust = bool(s["robust"])

    def robustify(self, chi2):
        if not self.robust:
            return chi2, np.ones_like(chi2)
        delta = np.where(self.stereo, DELTA[1], DELTA[0])
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def global_ba(s, order=None, stop_flag=False):
    """-> dict(ran, kf_out (K, 7) f64, pos_out (P, 3) f32, included, chi2, the counters of vsg_global_ba_result, and `trace`:
    per iteration the list of (rho, accepted, ok2) of its trials)."""
    K, P = len(s["kfs"]), len(s["slots"])
    Tin = np.asarray(s["Tcw"], F32).reshape(K, 7)
    pos_in = np.asarray(s["store_pos"], F32)[np.asarray(s["slots"], np.int64)].reshape(P, 3)
    fixed = np.asarray(s["fixed"]).astype(bool)
    off = np.asarray(s["obs_off"])
    E = int(off[-1]) if P else 0
    out = dict(ran=0, kf_out=Tin.astype(np.float64), pos_out=pos_in.copy(), included=(np.diff(off) > 0).astype(np.uint8),
               chi2=np.zeros(E), n_opt_kf=int((~fixed).sum()) if P else 0, n_fixed_kf=int(fixed.sum()) if P else 0, n_points=P,
               n_edges=E, trace=[])
    if P == 0 or E == 0 or stop_flag:
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
    out["chi2"] = g.chi2.copy()
    for k in g.opt_kf:
        out["kf_out"][k] = np.concatenate(est[k])
    out["pos_out"][g.vertex_pt] = X[g.vertex_pt].astype(F32)
    out.update(ran=1, n_mono=int((~g.stereo).sum()), n_stereo=int(g.stereo.sum()), iterations_run=its, trials_run=trials,
               stop_reason=stop, **{"lambda": lam}, chi2_initial=chi_initial, chi2_final=current)
    return out

"""Optimizer::OptimizeEssentialGraph, first overload (Optimizer.cc:2456-2734), restated in NumPy float64 from the reference's
sources, independently of csrc/vsg_essential_graph.h: the stand-in for g2o, which cannot be built here.

From: g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h: the exponential :67-134, map :136-139, log :141-216, inverse :219-222,
operator* :254-261), deltaR / skew (se3_ops.hpp), VertexSim3Expmap::oplusImpl and EdgeSim3::computeError
(types_seven_dof_expmap.h:62-71, :107-115), the numeric Jacobian of BaseBinaryEdge::linearizeOplus and
constructQuadraticForm (base_binary_edge.hpp:131-205, :55-86), OptimizationAlgorithmLevenberg::solve
(optimization_algorithm_levenberg.cpp:61-199) with setUserLambdaInit(1e-16), the measurements and the point correction of
Optimizer.cc (:2536-2551, :2568-2656, :2723-2728), and the walk that builds the edge list (:2529-2660, build_edges).

Everything is batched over edges with NumPy; the dense system is solved by an LDL^T without pivoting (`ldlt`) or by
numpy.linalg.solve (`numpy`, a member of the perturbation set).  `jitter` is another libm (log, acos, sin, cos, exp; sqrt is
exact) whose results differ by 0 or +-1 ulp: the other member.

Every error evaluation logs how close it came to a branch of Sim3::log(): the smallest |d - (1 - 1e-5)| and
||sigma| - 1e-5| of a run come back as min_d_dist / min_sigma_dist."""
import math

import numpy as np

EPS = 1e-5
DELTA = 1e-9
DBL_MAX = 1.7976931348623157e308
STOP_ITERATIONS, STOP_TERMINATE, STOP_BAD = 0, 1, 2


class Jitter:
    """Another libm: moves each result by 0 or +-1 ulp, by a seeded hash of the result's own bits, so that it stays a FUNCTION
    (the same argument gives the same result: the exactly-zero column of fix_scale rests on that, the two perturbed
    evaluations being the same computation).  Results that are exactly 0 or 1 stay: every libm returns exp(0) = 1,
    cos(0) = 1, log(1) = 0, sin(0) = 0 and acos(1) = 0 exactly."""

    def __init__(self, seed):
        self.seed = np.uint64((0x9E3779B97F4A7C15 * (2 * seed + 1)) & 0xFFFFFFFFFFFFFFFF)

    def __call__(self, v):
        v = np.ascontiguousarray(v, np.float64)
        with np.errstate(over="ignore"):
            z = v.view(np.uint64) + self.seed  # splitmix64
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        k = (z % np.uint64(3)).astype(np.int64) - 1
        out = np.where(k > 0, np.nextafter(v, np.inf), np.where(k < 0, np.nextafter(v, -np.inf), v))
        return np.where(np.isfinite(v) & (v != 0.0) & (v != 1.0), out, v)


def _same(v):
    return np.asarray(v, np.float64)


def _scalar(v):
    return float(np.asarray(v).reshape(-1)[0])


class Trace:
    def __init__(self):
        self.min_d, self.min_sigma = math.inf, math.inf

    def log(self, d, sigma):
        with np.errstate(invalid="ignore"):
            a, b = np.abs(d - (1 - EPS)), np.abs(np.abs(sigma) - EPS)
        a, b = a[np.isfinite(a)], b[np.isfinite(b)]
        if a.size:
            self.min_d = min(self.min_d, float(a.min()))
        if b.size:
            self.min_sigma = min(self.min_sigma, float(b.min()))


# ---- quaternions as Eigen has them (x y z w), batched over leading axes

def q_rotate(q, v):
    qv, w = q[..., :3], q[..., 3:4]
    uv = 2.0 * np.cross(qv, v)
    return v + w * uv + np.cross(qv, uv)


def q_mul(a, b):
    ax, ay, az, aw = (a[..., k] for k in range(4))
    bx, by, bz, bw = (b[..., k] for k in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def q_matrix(q):
    x, y, z, w = (q[..., k] for k in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def q_from_matrix(m):
    """Eigen's Quaternion(Matrix3d), one matrix."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    with np.errstate(invalid="ignore", divide="ignore"):
        if t > 0:
            t = math.sqrt(t + 1.0)
            q[3] = 0.5 * t
            t = 0.5 / t
            q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            a = m[i, i] - m[j, j] - m[k, k] + 1.0
            t = math.sqrt(a) if a >= 0 else math.nan
            q[i] = 0.5 * t
            t = 0.5 / t if t != 0 else math.inf
            q[3], q[j], q[k] = (m[k, j] - m[j, k]) * t, (m[j, i] + m[i, j]) * t, (m[k, i] + m[i, k]) * t
    return q


def skew(v):
    O = np.zeros(v.shape[:-1] + (3, 3))
    O[..., 0, 1], O[..., 0, 2], O[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    O[..., 1, 2], O[..., 2, 0], O[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return O


# ---- g2o::Sim3 as a tuple (q [..., 4], t [..., 3], s [...])

def sim3(a):
    a = np.asarray(a, np.float64)
    return a[..., :4].copy(), a[..., 4:7].copy(), a[..., 7].copy()


def pack(S):
    return np.concatenate([S[0], S[1], np.asarray(S[2])[..., None]], -1)


def s_map(S, x):
    return S[2][..., None] * q_rotate(S[0], x) + S[1]


def s_mul(a, b):
    return q_mul(a[0], b[0]), s_map(a, b[1]), a[2] * b[2]


def s_inv(a):
    qc = a[0] * np.array([-1.0, -1.0, -1.0, 1.0])
    return qc, q_rotate(qc, (-1.0 / a[2])[..., None] * a[1]), 1.0 / a[2]


def s_exp(u, jit=_same):
    """Sim3(const Vector7d &update), one update."""
    u = np.asarray(u, np.float64)
    omega, ups, sigma = u[:3], u[3:6], float(u[6])
    with np.errstate(all="ignore"):
        theta = math.sqrt(float(omega @ omega)) if np.isfinite(omega).all() else math.nan
        O = skew(omega)
        O2 = O @ O
        s = _scalar(jit(np.exp(sigma)))
        I = np.eye(3)
        small = theta < EPS
        if small:
            R = I + O + O2
            sn = cs = 0.0
        else:
            sn, cs = _scalar(jit(np.sin(theta))), _scalar(jit(np.cos(theta)))
            R = I + sn / theta * O + (1 - cs) / (theta * theta) * O2
        if abs(sigma) < EPS:
            C = 1.0
            if small:
                A, B = 1. / 2., 1. / 6.
            else:
                theta2 = theta * theta
                A, B = (1 - cs) / theta2, (theta - sn) / (theta2 * theta)
        else:
            C = (s - 1) / sigma
            if small:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            else:
                a, b, theta2, sigma2 = s * sn, s * cs, theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        W = A * O + B * O2 + C * I
        return q_from_matrix(R), W @ ups, np.float64(s)


def s_log(S, trace, jit=_same):
    """g2o::Sim3::log(), batched: [..., 7] = omega, upsilon, sigma."""
    q, t, s = S
    with np.errstate(all="ignore"):
        sigma = jit(np.log(s))
        R = q_matrix(q)
        d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
        trace.log(d, sigma)
        dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
        near, small = d > 1 - EPS, np.abs(sigma) < EPS
        theta = jit(np.arccos(d))
        sn, cs = jit(np.sin(theta)), jit(np.cos(theta))
        f = np.where(near, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        omega = f[..., None] * dR
        theta2, sigma2 = theta * theta, sigma * sigma
        C = np.where(small, 1.0, (s - 1) / sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma2
        A = np.where(small, np.where(near, 0.5, (1 - cs) / theta2),
                     np.where(near, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small, np.where(near, 1. / 6., (theta - sn) / (theta2 * theta)),
                     np.where(near, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma),
                              (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2))
        O = skew(omega)
        W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3)
        ups = np.full(t.shape, np.nan)
        flatW, flatt, flatu = W.reshape(-1, 3, 3), t.reshape(-1, 3), ups.reshape(-1, 3)
        for k in range(flatW.shape[0]):  # W.lu().solve(t): LAPACK's partial pivoting, as Eigen's PartialPivLU
            if np.isfinite(flatW[k]).all() and np.isfinite(flatt[k]).all():
                try:
                    flatu[k] = np.linalg.solve(flatW[k], flatt[k])
                except np.linalg.LinAlgError:
                    pass
        ups = flatu.reshape(t.shape)
        return np.concatenate([omega, ups, sigma[..., None]], -1)


def edge_error(C, v1, v2, trace, jit=_same):
    """EdgeSim3::computeError: (C * v1 * v2^-1).log()"""
    return s_log(s_mul(s_mul(C, v1), s_inv(v2)), trace, jit)


def take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


def measurements(Scw, nonc, has, ei, ej, eloop):
    """Sji = Sjw * Swi (:2536-2551, :2568-2656)"""
    V, N = sim3(Scw), sim3(nonc)
    use_i, use_j = (has[ei] != 0) & (eloop == 0), (has[ej] != 0) & (eloop == 0)
    side = lambda idx, use: tuple(np.where(use.reshape((-1,) + (1,) * (a.ndim - 1)), b[idx], a[idx]) for a, b in zip(V, N))
    return s_mul(side(ej, use_j), s_inv(side(ei, use_i)))


def ldlt_solve(A, b):
    n = len(b)
    L, D, ok = np.eye(n), np.zeros(n), True
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j] - np.sum(L[j, :j] * L[j, :j] * D[:j])
            D[j] = d
            if d <= 0.0:
                ok = False
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j] * D[:j]).sum(1)) / d
        y = np.zeros(n)
        for i in range(n):
            y[i] = b[i] - L[i, :i] @ y[:i]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = y[i] / D[i] - L[i + 1:, i] @ x[i + 1:]
    return x, ok


def numpy_solve(A, b):
    """The same decision (is the matrix positive definite?) by Cholesky, the solution by LAPACK."""
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return ldlt_solve(A, b)
    try:
        np.linalg.cholesky(A)
        ok = True
    except np.linalg.LinAlgError:
        ok = False
    try:
        return np.linalg.solve(A, b), ok
    except np.linalg.LinAlgError:
        return ldlt_solve(A, b)[0], ok


def correct_points(Scw, final, point_ref, pos):
    """:2723-2728: float(correctedSwr.map(Srw.map(double(pos))))"""
    ref = np.asarray(point_ref, np.int64)
    if ref.size == 0:
        return np.zeros((0, 3), np.float32)
    with np.errstate(all="ignore"):
        y = s_map(take(sim3(Scw), ref), np.asarray(pos, np.float32).astype(np.float64))
        return s_map(take(s_inv(sim3(final)), ref), y).astype(np.float32)


def optimize(Scw, nonc, has, fixed, ei, ej, eloop, fix_scale, iterations, jitter=None, solver="ldlt"):
    """Returns dict(kf_Scw (K, 8), chi2 per edge after the last computeActiveErrors, ran, accepted (one flag per trial),
    iterations_run, trials_run, stop_reason, lambda, chi2_initial, chi2_final, min_d_dist, min_sigma_dist)."""
    jit = jitter if jitter is not None else _same
    Scw, nonc = np.asarray(Scw, np.float64).reshape(-1, 8), np.asarray(nonc, np.float64).reshape(-1, 8)
    has, fixed = np.asarray(has, np.uint8), np.asarray(fixed, np.uint8)
    ei, ej, eloop = np.asarray(ei, np.int64), np.asarray(ej, np.int64), np.asarray(eloop, np.uint8)
    K, E = Scw.shape[0], ei.size
    trace = Trace()
    out = dict(kf_Scw=Scw.copy(), chi2=np.zeros(E), ran=0, accepted=[], iterations_run=0, trials_run=0, stop_reason=0,
               chi2_initial=0.0, chi2_final=0.0, min_d_dist=math.inf, min_sigma_dist=math.inf)
    out["lambda"] = 0.0
    deg = np.bincount(np.concatenate([ei, ej]), minlength=K) if E else np.zeros(K, np.int64)
    opt = np.flatnonzero((fixed == 0) & (deg > 0))
    if E == 0 or opt.size == 0:
        return out
    col = np.full(K, -1, np.int64)
    col[opt] = np.arange(opt.size)
    n = 7 * opt.size
    est = sim3(Scw)
    meas = measurements(Scw, nonc, has, ei, ej, eloop)
    pert = []
    for d in range(7):
        for sign in (1.0, -1.0):
            u = np.zeros(7)
            u[d] = sign * DELTA
            if fix_scale:
                u[6] = 0
            pert.append(s_exp(u, jit))

    def errors(e_):
        return edge_error(meas, take(e_, ei), take(e_, ej), trace, jit)

    def chi2_of(err):
        with np.errstate(all="ignore"):
            return np.einsum("ek,kl,el->e", err, np.eye(7), err)

    lam, ni, n_bad, stop = 0.0, 2.0, 0, None
    with np.errstate(all="ignore"):
        for it in range(iterations):
            err = errors(est)
            currentChi = float(chi2_of(err).sum())
            iniChi = currentChi
            J = np.zeros((2, E, 7, 7))
            for v, idx in enumerate((ei, ej)):
                for d in range(7):
                    e_pm = []
                    for sgn in range(2):
                        P = pert[2 * d + sgn]
                        moved = s_mul(tuple(np.broadcast_to(a, (E,) + np.shape(a)) for a in P), take(est, idx))
                        vi, vj = (moved, take(est, ej)) if v == 0 else (take(est, ei), moved)
                        e_pm.append(edge_error(meas, vi, vj, trace, jit))
                    J[v, :, :, d] = (1.0 / (2 * DELTA)) * (e_pm[0] - e_pm[1])
            H, b = np.zeros((n, n)), np.zeros(n)
            for e in range(E):  # constructQuadraticForm, edges in insertion order
                ci, cj = col[ei[e]], col[ej[e]]
                A, B, omega = J[0, e], J[1, e], np.eye(7)
                omega_r = -omega @ err[e]
                if ci >= 0:
                    AtO = A.T @ omega
                    b[7 * ci:7 * ci + 7] += A.T @ omega_r
                    H[7 * ci:7 * ci + 7, 7 * ci:7 * ci + 7] += AtO @ A
                    if cj >= 0:
                        H[7 * ci:7 * ci + 7, 7 * cj:7 * cj + 7] += AtO @ B
                        H[7 * cj:7 * cj + 7, 7 * ci:7 * ci + 7] += (AtO @ B).T
                if cj >= 0:
                    b[7 * cj:7 * cj + 7] += B.T @ omega_r
                    H[7 * cj:7 * cj + 7, 7 * cj:7 * cj + 7] += B.T @ omega @ B
            if it == 0:
                lam, ni, n_bad = 1e-16, 2.0, 0  # computeLambdaInit returns the user value
                out["chi2_initial"] = currentChi
            rho, qmax = 0.0, 0
            while True:
                x, ok2 = (numpy_solve if solver == "numpy" else ldlt_solve)(H + lam * np.eye(n), b)
                x = x.copy()
                cand = tuple(a.copy() for a in est)
                for a_, k in enumerate(opt):
                    u = x[7 * a_:7 * a_ + 7]
                    if fix_scale:
                        u[6] = 0  # in the solver's array: computeScale reads it
                    new = s_mul(s_exp(u, jit), take(est, k))
                    cand[0][k], cand[1][k], cand[2][k] = new
                tempChi = float(chi2_of(errors(cand)).sum())
                if not ok2:
                    tempChi = DBL_MAX
                rho = currentChi - tempChi
                scale = float(np.sum(x * (lam * x + b))) + 1e-3
                rho = rho / scale
                accepted = bool(rho > 0 and math.isfinite(tempChi))
                if accepted:
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni, currentChi, est = 2.0, tempChi, cand
                else:
                    lam *= ni
                    ni *= 2
                out["accepted"].append(accepted)
                qmax += 1
                out["trials_run"] += 1
                if not (rho < 0 and qmax < 10):
                    break
            out["iterations_run"] += 1
            if qmax == 10 or rho == 0:
                stop = STOP_TERMINATE
                break
            n_bad = n_bad + 1 if (iniChi - currentChi) * 1e3 < iniChi else 0
            if n_bad >= 3:
                stop = STOP_BAD
                break
        final = pack(est)
        out["chi2"] = chi2_of(errors(est))  # computeActiveErrors of :2685
    out["kf_Scw"][opt] = final[opt]
    out.update(ran=1, stop_reason=STOP_ITERATIONS if stop is None else stop, chi2_final=currentChi,
               min_d_dist=trace.min_d, min_sigma_dist=trace.min_sigma)
    out["lambda"] = lam
    return out


def build_edges(parent, loops, children, covisibles, loop_connections, cur, loop_kf, min_feat=100):
    """The walk of Optimizer.cc:2529-2660 over keyframes named by their index in ascending mnId (-1: a bad keyframe).
    loops / children / covisibles: one list per keyframe; loop_connections: a list of (keyframe, [(connection, weight), ...])
    in the map's iteration order.  Returns (edge_i, edge_j, edge_loop)."""
    ei, ej, el, inserted = [], [], [], set()
    for i, conns in loop_connections:
        for j, w in conns:
            if j < 0 or j == i:
                continue
            if (i != cur or j != loop_kf) and w < min_feat:  # :2542
                continue
            ei.append(i), ej.append(j), el.append(1)
            inserted.add((min(i, j), max(i, j)))
    for i in range(len(parent)):
        p = parent[i]
        if p >= 0 and p != i:
            ei.append(i), ej.append(p), el.append(0)
        for l in loops[i]:
            if 0 <= l < i:  # :2608
                ei.append(i), ej.append(l), el.append(0)
        for c in covisibles[i]:
            if c >= 0 and c != p and c not in children[i] and c < i:  # :2634-2637
                if (min(i, c), max(i, c)) in inserted:
                    continue
                ei.append(i), ej.append(c), el.append(0)
    return np.array(ei, np.int32), np.array(ej, np.int32), np.array(el, np.uint8)

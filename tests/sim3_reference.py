"""NumPy restatement of the REFERENCE path of Sim3Solver (Sim3Solver.cc), for the tests of csrc/vsg_sim3.h: float32 throughout,
numpy.linalg.eig on the float32 N as the stand-in for Eigen::EigenSolver<Matrix4f> (LAPACK's general solver in single
precision), atan2 + Rodrigues in float32 for Sophus::SO3f::exp, the truncated thresholds, and iterate's loop transcribed
literally.  Each quirk has a switch that "fixes" it, so that a test can show the header keeps the quirk."""
import math

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32


def max_err(sigma2, truncated=True):
    """mvnMaxError (:96-97): 9.210 * sigmaSquare is a double pushed into a std::vector<size_t>, compared after a conversion to
    float.  truncated=False: the threshold a reader expects."""
    t = 9.210 * np.asarray(sigma2, F32).astype(F64)
    return (np.floor(t) if truncated else t).astype(F32)


def level_sigma2(nlevels=8, scale_factor=1.2):
    """mvLevelSigma2 as ORBextractor fills it: float products."""
    sf = [F32(1.0)]
    for _ in range(1, nlevels):
        sf.append(F32(sf[-1] * F32(scale_factor)))
    return np.array([F32(s * s) for s in sf], F32)


def project(cam, X):
    X = np.asarray(X, F32).reshape(-1, 3)
    return np.stack([F32(cam["fx"]) * X[:, 0] / X[:, 2] + F32(cam["cx"]), F32(cam["fy"]) * X[:, 1] / X[:, 2] + F32(cam["cy"])], 1)


def set_up(kf1, kf2, Xw1, Xw2, pose2=None):
    """:103-115.  pose2: the pose X3Dc2 goes through; the reference uses pKF2's also for a point matched through another
    keyframe.  Returns X3Dc1, X3Dc2, P1im1, P2im2 (float32)."""
    p2 = kf2 if pose2 is None else pose2
    X1 = (np.asarray(Xw1, F32) @ kf1["Rcw"].astype(F32).T + kf1["tcw"].astype(F32)).astype(F32)
    X2 = (np.asarray(Xw2, F32) @ p2["Rcw"].astype(F32).T + p2["tcw"].astype(F32)).astype(F32)
    return X1, X2, project(kf1, X1), project(kf2, X2)


def horn_n(P1, P2):
    """Centroids, M and N of :319-345.  P1 / P2: 3 x 3 float32 with the sampled points as COLUMNS."""
    P1, P2 = np.asarray(P1, F32), np.asarray(P2, F32)
    O1, O2 = (P1.sum(1) / F32(3)).astype(F32), (P2.sum(1) / F32(3)).astype(F32)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = (Pr2 @ Pr1.T).astype(F32)
    N11, N12, N13, N14 = M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
    N22, N23, N24 = M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
    N33, N34, N44 = -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], F32)
    return O1, O2, Pr1, Pr2, N


def rodrigues(v):
    """Sophus::SO3f::exp(v).matrix() as Rodrigues' formula in float32."""
    v = np.asarray(v, F32)
    th = F32(np.sqrt((v * v).sum(dtype=F32)))
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], F32)
    if th < F32(1e-5):
        return (np.eye(3, dtype=F32) + K + F32(0.5) * (K @ K)).astype(F32)
    a, b = F32(np.sin(th) / th), F32((F32(1) - np.cos(th)) / (th * th))
    return (np.eye(3, dtype=F32) + a * K + b * (K @ K)).astype(F32)


def compute_sim3(P1, P2, fix_scale=False, nan_on_zero_axis=True):
    """ComputeSim3 (:307-407).  nan_on_zero_axis=False "fixes" :362: a zero imaginary part gives the identity rotation
    instead of 0 / 0."""
    O1, O2, Pr1, Pr2, N = horn_n(P1, P2)
    with np.errstate(all="ignore"):
        ev, evec = np.linalg.eig(N)
        ev, evec = np.real(ev).astype(F32), np.real(evec).astype(F32)
        order = np.sort(ev)[::-1]
        gap = float((order[0] - order[1]) / max(abs(float(order[0])), 1e-30))
        q = evec[:, int(np.argmax(ev))]
        vec = q[1:4].astype(F32)
        nv = F32(np.sqrt((vec * vec).sum(dtype=F32)))
        ang = math.atan2(float(nv), float(q[0]))
        if nv == 0 and not nan_on_zero_axis:
            R = np.eye(3, dtype=F32)
        else:
            R = rodrigues(F32(2 * ang) * vec / nv)
        P3 = (R @ Pr2).astype(F32)
        if fix_scale:
            s = F32(1.0)
        else:
            s = F32(float((Pr1 * P3).sum(dtype=F32)) / float((P3 * P3).sum(dtype=F32)))
        sR = (s * R).astype(F32)
        t = (O1 - sR @ O2).astype(F32)
        sRinv = (F32(1.0 / float(s)) * R.T).astype(F32)
        T12, T21 = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
        T12[:3, :3], T12[:3, 3] = sR, t
        T21[:3, :3], T21[:3, 3] = sRinv, (-(sRinv @ t)).astype(F32)
    return dict(R=R, t=t, s=s, T12=T12, T21=T21, N=N, gap=gap)


def errors(h, kf1, kf2, X1, X2, p1, p2):
    """err1, err2 of CheckInliers (:412-423) for every correspondence."""
    with np.errstate(all="ignore"):
        a = project(kf1, (X2 @ h["T12"][:3, :3].T + h["T12"][:3, 3]).astype(F32))
        b = project(kf2, (X1 @ h["T21"][:3, :3].T + h["T21"][:3, 3]).astype(F32))
        d1, d2 = (p1 - a).astype(F32), (b - p2).astype(F32)
        return (d1 * d1).sum(1, dtype=F32), (d2 * d2).sum(1, dtype=F32)


def inliers(err1, err2, max1, max2):
    with np.errstate(invalid="ignore"):
        return (err1 < max1) & (err2 < max2)


def iterate_transcribed(counts, min_inliers, max_its, chunk=20):
    """iterate (:215-291) called `while (!bConverge && !bNoMore)` with nIterations = chunk, over given inlier counts: returns
    (best k or -1, bConverge, bNoMore, mnIterations, mnBestInliers)."""
    mnIterations, mnBestInliers, best = 0, 0, -1
    bConverge = bNoMore = False
    while not bConverge and not bNoMore:
        nCurrent = 0
        while mnIterations < max_its and nCurrent < chunk:
            nCurrent += 1
            mnIterations += 1
            c = int(counts[mnIterations - 1])
            if c >= mnBestInliers:
                mnBestInliers, best = c, mnIterations - 1
                if c > min_inliers:
                    bConverge = True
                    break
        if not bConverge and mnIterations >= max_its:
            bNoMore = True
    return best, bConverge, bNoMore, mnIterations, mnBestInliers


def ransac_iterations(probability, min_inliers, max_iterations, n):
    """SetRansacParameters (:120-144)."""
    epsilon = F32(F32(min_inliers) / F32(n))
    if min_inliers == n:
        it = 1
    else:
        it = int(math.ceil(math.log(1 - probability) / math.log(1 - float(epsilon) ** 3)))
    return max(1, min(it, max_iterations))


def draw_samples(n, n_hyp, random_int):
    """:242-256 written out: random_int(lo, hi) is DUtils::Random::RandomInt."""
    out = np.zeros((n_hyp, 3), I32)
    for k in range(n_hyp):
        avail = list(range(n))
        for i in range(3):
            r = random_int(0, len(avail) - 1)
            out[k, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out

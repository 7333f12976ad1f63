"""A NumPy float64 restatement of MLPnPsolver (MLPnPsolver.cpp): the constructor's arithmetic, SetRansacParameters, computePose
with its Gauss-Newton, CheckInliers and iterate as the SEQUENTIAL loop, state and all.  numpy.linalg.svd / eigh / solve and
libm where the library runs its own Jacobi, LDL^T, acos and cube root: what tests/test_mlpnp_reference.py measures the host
build of csrc/vsg_mlpnp.h against.  The Jacobian is written independently of the header's, through the right Jacobian of
SO(3): d(R(w) X)/dw = -R [X]x Jr(w)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS = np.finfo(F64).eps


def make_points(cam, kx, ky, octave, world_pos, slots, level_sigma2, th2):
    """The constructor (:55-101) and mvMaxError (:266) for the features with a slot, in feature order."""
    fx, fy, cx, cy = (F32(v) for v in cam)
    keep = np.flatnonzero(np.asarray(slots) >= 0)
    u, v = np.asarray(kx, F32)[keep], np.asarray(ky, F32)[keep]
    bear = np.stack([((u - cx) / fx).astype(F64), ((v - cy) / fy).astype(F64), np.ones(len(keep))], 1)
    X = np.asarray(world_pos, F32)[np.asarray(slots)[keep]]
    max_err = (np.asarray(level_sigma2, F32)[np.asarray(octave)[keep]] * F32(th2)).astype(F32)
    return dict(u=u, v=v, f=bear, X=X.astype(F64), Xf=X, max_err=max_err, feat=keep, cam=(fx, fy, cx, cy))


def ransac_parameters(probability, min_inliers, max_iterations, min_set, epsilon, n):
    """SetRansacParameters (:231-262): returns (mRansacMinInliers, mRansacMaxIts)."""
    eps = F32(epsilon)
    m = int(F32(n) * eps)
    m = max(m, min_inliers, min_set)
    with np.errstate(divide="ignore", invalid="ignore"):
        if eps < F32(m) / F32(n):
            eps = F32(m) / F32(n)
        if m == n:
            its = 1
        else:
            v = np.ceil(np.log(1 - F64(probability)) / np.log(1 - F64(eps) ** 3))
            its = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31
    return m, max(1, min(its, max_iterations))


def draw_sets(n, n_hyp, random_int):
    out = np.zeros((n_hyp, 6), np.int32)
    for k in range(n_hyp):
        avail = list(range(n))
        for i in range(6):
            r = random_int(0, len(avail) - 1)
            out[k, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], F64)


def rodrigues2rot(w):
    n = np.linalg.norm(w)
    if n > EPS:
        K = skew(w)
        return np.eye(3) + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return np.eye(3)


def rot2rodrigues(R, fix_acos=False):
    c = (np.trace(R) - 1.0) / 2.0
    if fix_acos:
        c = min(1.0, max(-1.0, c))
    wn = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")  # out of range: NaN, `wnorm > eps` is false, omega = 0
    if wn > EPS:
        return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))
    return np.zeros(3)


def nullspaces(f):
    out = np.zeros((len(f), 3, 2))
    for i, b in enumerate(f):
        out[i] = np.linalg.svd(b.reshape(1, 3))[2].T[:, 1:3]
    return out


def residuals_and_jacs(x, X, ns):
    w, t = x[:3], x[3:]
    R = rodrigues2rot(w)
    th = np.linalg.norm(w)
    if th > EPS:
        K = skew(w)
        Jr = np.eye(3) - (1 - math.cos(th)) / th ** 2 * K + (th - math.sin(th)) / th ** 3 * (K @ K)
    else:
        Jr = np.eye(3)  # the limit: the header pins it, the reference divides by |w|
    r, J = np.zeros(2 * len(X)), np.zeros((2 * len(X), 6))
    for i in range(len(X)):
        p = R @ X[i] + t
        ln = np.linalg.norm(p)
        v = p / ln
        D = (np.eye(3) - np.outer(v, v)) / ln
        dp = np.hstack([-R @ skew(X[i]) @ Jr, np.eye(3)])
        r[2 * i:2 * i + 2] = ns[i].T @ v
        J[2 * i:2 * i + 2] = ns[i].T @ D @ dp
    return r, J


def gauss_newton(x, X, ns, keep_x_on_abort=True):
    info = dict(rounds=0, aborted=False, max_dx=0.0, min_dx=0.0, max_dl=0.0, margins=[])
    x = x.copy()
    for _ in range(5):
        r, J = residuals_and_jacs(x, X, ns)
        with np.errstate(all="ignore"):
            try:
                dx = np.linalg.solve(J.T @ J, J.T @ r)
            except np.linalg.LinAlgError:
                dx = np.full(6, np.nan)
        a = np.abs(dx)
        info["rounds"] += 1
        info["max_dx"], info["min_dx"] = a.max(), a.min()
        info["margins"] += [(a.max(), 5.0), (a.min(), 1.0)]
        if a.max() > 5.0 or a.min() > 1.0:
            info["aborted"] = True
            if not keep_x_on_abort:
                x = x - dx
            break
        dl = np.abs(J @ dx).max()
        info["max_dl"] = dl
        info["margins"].append((dl, 1e-5))
        x = x - dx
        if dl < 1e-5:
            break
    return x, info


def signed_eigenvectors(M):
    """Rows = eigenvectors in ascending eigenvalue order, each with its largest component positive (the header's pin)."""
    E = np.linalg.eigh(M)[1].T.copy()
    for r in E:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1
    return E


def compute_pose(f, X, fix_acos=False, keep_x_on_abort=True):
    """computePose (:365-683) on bearings f [m, 3] and points X [m, 3].  Returns R, t, info."""
    m = len(X)
    ns = nullspaces(f)
    M = X.T @ X
    sv = np.linalg.svd(M, compute_uv=False)
    planar = int((sv > 3 * EPS * sv[0]).sum()) == 2
    E = signed_eigenvectors(M) if planar else np.eye(3)
    P = X @ E.T
    A = np.zeros((2 * m, 9 if planar else 12))
    for i in range(m):
        for h in range(2):
            n = ns[i][:, h]
            if planar:
                A[2 * i + h] = np.concatenate([np.outer(n, P[i, 1:]).ravel(), n])
            else:
                A[2 * i + h] = np.concatenate([np.outer(n, P[i]).ravel(), n])
    AtA = A.T @ A
    U, S, Vt = np.linalg.svd(AtA)
    v = Vt[-1]
    info = dict(planar=planar, gap=(S[-2] - S[-1]) / S[0] if S[0] > 0 else 0.0)
    with np.errstate(all="ignore"):
        if planar:
            tmp = np.zeros((3, 3))
            tmp[:, 1], tmp[:, 2] = v[0:6:2], v[1:6:2]
            tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
            tmp = tmp.T.copy()
            scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            U3, _, V3t = np.linalg.svd(tmp)
            R1 = U3 @ V3t
            if np.linalg.det(R1) < 0:
                R1 = -R1
            R1 = E.T @ R1
            t = scale * v[6:9]
            R1 = -R1.T
            if np.linalg.det(R1) < 0:
                R1[:, 2] *= -1
            R2 = R1 * np.array([-1.0, -1.0, 1.0])
            cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
        else:
            tmp = v[:9].reshape(3, 3).T.copy()
            scale = 1.0 / abs(np.prod(np.linalg.norm(tmp, axis=0))) ** (1.0 / 3.0)
            U3, _, V3t = np.linalg.svd(tmp)
            Rout = U3 @ V3t
            if np.linalg.det(Rout) < 0:
                Rout = -Rout
            tout = Rout @ (scale * v[9:12])
            cands = [(Rout.T, -Rout.T @ tout), (Rout.T, Rout.T @ tout)]
        errs = []
        for Rc, tc in cands:
            e = 0.0
            for p in range(6):
                y = Rc @ X[p] + tc
                e += 1.0 - (y / np.linalg.norm(y)) @ f[p]
            errs.append(e)
    pick = int(np.argmin(errs)) if planar else (0 if errs[0] < errs[1] else 1)
    order = np.sort(errs)
    info["direction"] = (order[0], order[1])
    Rsel, tsel = cands[pick]
    x0 = np.concatenate([rot2rodrigues(Rsel, fix_acos), tsel])
    info["x0"] = x0
    x, gn = gauss_newton(x0, X, ns, keep_x_on_abort)
    info["gn"] = gn
    return rodrigues2rot(x[:3]), x[3:], info


def check_inliers(pts, R, t, depth_test=False):
    """CheckInliers (:269-301): flags and the squared errors in float32."""
    fx, fy, cx, cy = pts["cam"]
    X = pts["Xf"].astype(F64)
    with np.errstate(all="ignore"):
        c = [(((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r]).astype(F32) for r in range(3)]
        u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
        dx, dy = pts["u"] - u, pts["v"] - v
        e2 = (dx * dx + dy * dy).astype(F32)
        ok = e2 < pts["max_err"]
    if depth_test:
        ok &= c[2] > 0
    return ok, e2


class Solver:
    """The solver with its members; iterate is the reference's loop.  `variant` switches ONE behaviour to its "fix" for
    tests/test_mlpnp_quirks.py: gate_strict, refine_installs, last_max, and_loop, no_more_at_last, refined_on_no_more,
    depth_test, fix_acos, abort_applies."""

    def __init__(self, pts, sets, min_inliers, max_its, variant=None):
        self.pts, self.sets, self.min_inliers, self.max_its, self.variant = pts, np.asarray(sets), min_inliers, max_its, variant
        self.N = len(pts["u"])
        self.iterations, self.best_count, self.best_flags, self.best_T, self.best_k = 0, 0, None, None, -1
        self.refines = 0

    def pose_of(self, idx):
        return compute_pose(self.pts["f"][idx], self.pts["X"][idx], fix_acos=self.variant == "fix_acos",
                            keep_x_on_abort=self.variant != "abort_applies")

    def check(self, R, t):
        return check_inliers(self.pts, R, t, depth_test=self.variant == "depth_test")[0]

    def refine(self, flags):
        """Refine() (:303-362) as its code has it: computePose over the best set goes into a LOCAL `result` that is never
        copied into mRi / mti, so CheckInliers() at :340 runs on the pose of the hypothesis just computed.  The variant
        refine_installs copies it, which is what the routine's name promises."""
        self.refines += 1
        R, t, _ = self.pose_of(np.flatnonzero(flags))
        if self.variant in ("refine_installs", "refined_on_no_more"):
            self.mRi, self.mti = R, t
        fl = self.check(self.mRi, self.mti)
        return int(fl.sum()) > self.min_inliers, self.mRi, self.mti, fl

    def iterate(self, n_iterations):
        """Returns dict(found, no_more, inlier, n_inliers, T, refined)."""
        out = dict(found=False, no_more=False, inlier=np.zeros(self.N, bool), n_inliers=0, T=np.eye(4), refined=False)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        v = self.variant
        while (self.iterations < self.max_its and cur < n_iterations) if v == "and_loop" else \
                (self.iterations < self.max_its or cur < n_iterations):
            cur += 1
            k = self.iterations
            self.iterations += 1
            R, t, _ = self.pose_of(self.sets[k])
            self.mRi, self.mti = R, t  # :157-171
            fl = self.check(R, t)
            c = int(fl.sum())
            if (c > self.min_inliers) if v == "gate_strict" else (c >= self.min_inliers):
                if (c >= self.best_count) if v == "last_max" else (c > self.best_count):
                    self.best_flags, self.best_count, self.best_T, self.best_k = fl, c, (R, t), k
                ok, Rr, tr, flr = self.refine(self.best_flags)
                if ok:
                    last = self.iterations >= self.max_its and cur >= n_iterations
                    out.update(found=True, inlier=flr, n_inliers=int(flr.sum()), T=pose4(Rr, tr), refined=True,
                               no_more=bool(v == "no_more_at_last" and last))
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
            if self.best_count >= self.min_inliers:
                R, t = self.best_T
                fl = self.best_flags
                if v == "refined_on_no_more":
                    _, R, t, fl = self.refine(self.best_flags)
                out.update(found=True, inlier=fl, n_inliers=int(fl.sum()), T=pose4(R, t))
        return out


def pose4(R, t):
    T = np.eye(4, dtype=F32)
    T[:3, :3], T[:3, 3] = R.astype(F32), t.astype(F32)
    return T


def loop_on_counts(c, first, n_iterations, max_its, min_inliers, variant=None, best_set_count=None):
    """iterate's loop (:120-228) on the hypotheses' inlier counts alone, replayed from hypothesis 0 so that the members hold
    what earlier calls left.  Refine() at hypothesis k counts the inliers of hypothesis k's pose again, so it succeeds iff
    c[k] > min_inliers and returns hypothesis k.  Returns dict(found, no_more, refined, best, iterations, pose, records): pose =
    the hypothesis whose pose and flags are returned.  variant as in Solver; refine_installs takes best_set_count[b] = the
    inliers of the pose solved over the best set b and returns that pose (pose = -2)."""
    v = variant
    it, best, best_c, records = 0, -1, 0, 0
    out = None
    calls = [(first, 0), (n_iterations, 1)] if first else [(n_iterations, 1)]
    for n_it, real in calls:  # the calls before `first` are replayed as one that walks to `first` without returning
        cur = 0
        while ((it < max_its and cur < n_it) if v == "and_loop" else (it < max_its or cur < n_it)) if real else it < first:
            cur += 1
            k = it
            it += 1
            if (c[k] > min_inliers) if v == "gate_strict" else (c[k] >= min_inliers):
                if (c[k] >= best_c) if v == "last_max" else (c[k] > best_c):
                    best, best_c, records = k, c[k], records + 1
                ok = best_set_count[best] > min_inliers if v == "refine_installs" else c[k] > min_inliers
                if real and ok:
                    last = it >= max_its and cur >= n_it
                    return dict(found=1, no_more=int(v == "no_more_at_last" and last), refined=1, best=best, iterations=it,
                                pose=-2 if v == "refine_installs" else k, records=records)
        out = dict(found=0, no_more=0, refined=0, best=best, iterations=it, pose=-1, records=records)
        if real and it >= max_its:
            out["no_more"] = 1
            if best_c >= min_inliers:
                out["found"], out["pose"] = 1, best
                out["refined"] = int(v == "refined_on_no_more")
    return out

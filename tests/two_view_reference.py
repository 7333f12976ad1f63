"""TwoViewReconstruction::Reconstruct restated in NumPy float32, statement by statement (TwoViewReconstruction.cc; the
line numbers are its).  numpy.linalg.svd on the float32 systems stands in for Eigen's JacobiSVD, numpy.linalg.inv for
Matrix3f::inverse().  Loops over the matches are written as float32 array expressions (one rounding per operation, as the
scalar code) and the score as a float32 cumulative sum, which adds in index order."""
import numpy as np

F32, F64 = np.float32, np.float64


def _f(v):
    return np.asarray(v, F32)


def _inv_double(x):
    """1.0 / x with a float x: the double quotient rounded to float"""
    return (F64(1.0) / np.asarray(x, F64)).astype(F32)


def normalize(xy, over=None):
    """Normalize (:735-782) over ALL keypoints.  Returns (normalised points [n, 2], T)."""
    xy = _f(xy)
    n = len(xy)
    src = xy if over is None else _f(over)  # `over`: the restatement that "fixes" the quirk sums other points
    m = len(src)
    meanX = np.cumsum(src[:, 0], dtype=F32)[-1] / F32(m)
    meanY = np.cumsum(src[:, 1], dtype=F32)[-1] / F32(m)
    devX = np.cumsum(np.abs(src[:, 0] - meanX), dtype=F32)[-1] / F32(m)
    devY = np.cumsum(np.abs(src[:, 1] - meanY), dtype=F32)[-1] / F32(m)
    sX, sY = _inv_double(devX), _inv_double(devY)
    pn = np.stack([(xy[:, 0] - meanX) * sX, (xy[:, 1] - meanY) * sY], 1).astype(F32)
    T = np.zeros((3, 3), F32)
    T[0, 0], T[1, 1], T[0, 2], T[1, 2], T[2, 2] = sX, sY, -meanX * sX, -meanY * sY, 1
    assert n == len(pn)
    return pn, T


def system_h(p1, p2):
    """A of ComputeH21 (:235-263), float32 16 x 9"""
    A = np.zeros((16, 9), F32)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -u1, -v1, -1
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = v2 * u1, v2 * v1, v2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = u1, v1, 1
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -u2 * u1, -u2 * v1, -u2
    return A


def system_f(p1, p2):
    """A of ComputeF21 (:276-294), float32 8 x 9"""
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(8, F32)], 1).astype(F32)


def compute_h21(p1, p2):
    _, _, vt = np.linalg.svd(system_h(p1, p2), full_matrices=True)
    return vt[8].reshape(3, 3).astype(F32)


def compute_f21(p1, p2):
    _, _, vt = np.linalg.svd(system_f(p1, p2), full_matrices=True)
    Fpre = vt[8].reshape(3, 3).astype(F32)
    u, w, vt2 = np.linalg.svd(Fpre)
    w = w.astype(F32)
    w[2] = 0
    return (u.astype(F32) @ np.diag(w) @ vt2.astype(F32)).astype(F32)


def check_homography(H21, H12, m, sigma, th=5.991):
    """CheckHomography (:308-391) on the matches m [N, 4] = {u1, v1, u2, v2}.  Returns (score, inliers, terms, chi [N, 2])."""
    th = F32(th)
    inv = _inv_double(F32(sigma) * F32(sigma))
    u1, v1, u2, v2 = (m[:, k] for k in range(4))
    h, g = _f(H21), _f(H12)
    w2 = _inv_double(g[2, 0] * u2 + g[2, 1] * v2 + g[2, 2])
    u2in1, v2in1 = (g[0, 0] * u2 + g[0, 1] * v2 + g[0, 2]) * w2, (g[1, 0] * u2 + g[1, 1] * v2 + g[1, 2]) * w2
    chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv
    w1 = _inv_double(h[2, 0] * u1 + h[2, 1] * v1 + h[2, 2])
    u1in2, v1in2 = (h[0, 0] * u1 + h[0, 1] * v1 + h[0, 2]) * w1, (h[1, 0] * u1 + h[1, 1] * v1 + h[1, 2]) * w1
    chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv
    return _score(chi1, chi2, th, th)


def check_fundamental(F21, m, sigma, th=3.841, th_score=5.991):
    """CheckFundamental (:393-471): the gate at 3.841, the score against 5.991"""
    th, th_score = F32(th), F32(th_score)
    inv = _inv_double(F32(sigma) * F32(sigma))
    u1, v1, u2, v2 = (m[:, k] for k in range(4))
    f = _f(F21)
    a2, b2, c2 = f[0, 0] * u1 + f[0, 1] * v1 + f[0, 2], f[1, 0] * u1 + f[1, 1] * v1 + f[1, 2], f[2, 0] * u1 + f[2, 1] * v1 + f[2, 2]
    num2 = a2 * u2 + b2 * v2 + c2
    chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
    a1, b1, c1 = f[0, 0] * u2 + f[1, 0] * v2 + f[2, 0], f[0, 1] * u2 + f[1, 1] * v2 + f[2, 1], f[0, 2] * u2 + f[1, 2] * v2 + f[2, 2]
    num1 = a1 * u1 + b1 * v1 + c1
    chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
    return _score(chi1, chi2, th, th_score)


def _score(chi1, chi2, th, th_score):
    with np.errstate(invalid="ignore"):
        out1, out2 = chi1 > th, chi2 > th
    t = np.stack([np.where(out1, F32(0), th_score - chi1), np.where(out2, F32(0), th_score - chi2)], 1).astype(F32)
    score = np.cumsum(t.reshape(-1), dtype=F32)[-1] if len(t) else F32(0)
    return F32(score), ~(out1 | out2), t, np.stack([chi1, chi2], 1)


def first_maximum(scores):
    """The loops :155-178 / :205-228 over the scores: (winner or -1, score)"""
    best, s = -1, F32(0)
    for it, c in enumerate(scores):
        if c > s:
            best, s = it, c
    return best, s


def matches_of(xy1, xy2, matches12):
    i1 = np.nonzero(np.asarray(matches12) >= 0)[0]
    return i1, np.asarray(matches12)[i1]


def find(model, xy1, xy2, i1, i2, sets, sigma, normalize_over_matches=False, th_f=3.841):
    """FindHomography / FindFundamental: dict(M21 [n_iter], score [n_iter], inlier [n_iter, N], chi [n_iter, N, 2])"""
    if normalize_over_matches:
        pn1, T1 = normalize(xy1, over=_f(xy1)[i1])
        pn2, T2 = normalize(xy2, over=_f(xy2)[i2])
    else:
        pn1, T1 = normalize(xy1)
        pn2, T2 = normalize(xy2)
    m = np.concatenate([_f(xy1)[i1], _f(xy2)[i2]], 1)
    T2inv, T2t = np.linalg.inv(T2).astype(F32), T2.T.copy()
    out = dict(M21=[], M12=[], score=[], inlier=[], chi=[], T1=T1, T2=T2)
    for st in np.asarray(sets).reshape(-1, 8):
        p1, p2 = pn1[i1[st]], pn2[i2[st]]
        with np.errstate(all="ignore"):
            try:
                if model == 0:
                    H21 = (T2inv @ compute_h21(p1, p2) @ T1).astype(F32)
                    H12 = np.linalg.inv(H21).astype(F32)
                    sc, inl, _, chi = check_homography(H21, H12, m, sigma)
                    out["M12"].append(H12)
                else:
                    H21 = (T2t @ compute_f21(p1, p2) @ T1).astype(F32)
                    sc, inl, _, chi = check_fundamental(H21, m, sigma, th=th_f)
            except np.linalg.LinAlgError:
                H21, sc, inl, chi = np.full((3, 3), np.nan, F32), F32(np.nan), np.zeros(len(m), bool), np.full((len(m), 2), np.nan, F32)
        out["M21"].append(H21), out["score"].append(sc), out["inlier"].append(inl), out["chi"].append(chi)
    for k in ("M21", "score", "inlier", "chi"):
        out[k] = np.array(out[k])
    return out


def triangulate(x1, x2, P1, P2):
    """GeometricTools::Triangulate (GeometricTools.cc:47-66); None where x3Dh(3) == 0"""
    A = np.stack([x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1], x2[0] * P2[2] - P2[0], x2[1] * P2[2] - P2[1]]).astype(F32)
    _, _, vt = np.linalg.svd(A)
    h = vt[3].astype(F32)
    if h[3] == 0:
        return None
    return (h[:3] / h[3]).astype(F32)


def check_rt(R, t, m, first, inliers, K, n1, th2, flag_all_counted=False, index_rule=50):
    """CheckRT (:784-898): (nGood, vP3D [n1, 3], vbGood [n1], parallax, cosines, counted [N])"""
    R, t, K = _f(R), _f(t), _f(K)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    good, P3D, cosines = np.zeros(n1, bool), np.zeros((n1, 3), F32), []
    counted = np.zeros(len(m), bool)
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = K
    P2 = (K @ np.concatenate([R, t.reshape(3, 1)], 1)).astype(F32)
    O2 = (-R.T @ t).astype(F32)
    nGood = 0
    with np.errstate(all="ignore"):
        for i in range(len(m)):
            if not inliers[i]:
                continue
            u1, v1, u2, v2 = m[i]
            p = triangulate(_f([u1, v1, 1]), _f([u2, v2, 1]), P1, P2)
            if p is None or not np.all(np.isfinite(p)):
                continue
            n1v, n2v = p, (p - O2).astype(F32)
            d1, d2 = F32(np.sqrt(F32(n1v @ n1v))), F32(np.sqrt(F32(n2v @ n2v)))
            cosP = F32(F32(n1v @ n2v) / (d1 * d2))
            if p[2] <= 0 and F64(cosP) < 0.99998:
                continue
            p2 = (R @ p + t).astype(F32)
            if p2[2] <= 0 and F64(cosP) < 0.99998:
                continue
            iz1 = _inv_double(p[2])
            e1 = (fx * p[0] * iz1 + cx - u1) ** 2 + (fy * p[1] * iz1 + cy - v1) ** 2
            if e1 > th2:
                continue
            iz2 = _inv_double(p2[2])
            e2 = (fx * p2[0] * iz2 + cx - u2) ** 2 + (fy * p2[1] * iz2 + cy - v2) ** 2
            if e2 > th2:
                continue
            cosines.append(cosP)
            P3D[first[i]] = p
            nGood += 1
            counted[i] = True
            if flag_all_counted or F64(cosP) < 0.99998:
                good[first[i]] = True
    if nGood > 0:
        srt = np.sort(_f(cosines))
        idx = min(index_rule, len(srt) - 1) if index_rule is not None else len(srt) // 2
        parallax = F32(F64(F32(np.arccos(srt[idx])) * F32(180)) / np.pi)
    else:
        parallax = F32(0)
    return nGood, P3D, good, parallax, _f(cosines), counted


def decompose_e(E):
    u, _, vt = np.linalg.svd(_f(E))
    u, vt = u.astype(F32), vt.astype(F32)
    t = u[:, 2] / F32(np.linalg.norm(u[:, 2]))
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    R1, R2 = (u @ W @ vt).astype(F32), (u @ W.T @ vt).astype(F32)
    if np.linalg.det(R1) < 0:
        R1 = -R1
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return R1, R2, t.astype(F32)


def reconstruct_f(inl, F21, K, m, first, n1, sigma, min_parallax, min_tri):
    """ReconstructF (:473-570): dict(ok, reason, R, t, P3D, tri, n_good, parallax, N)"""
    N = int(np.sum(inl))
    K = _f(K)
    R1, R2, t = decompose_e((K.T @ _f(F21) @ K).astype(F32))
    th2 = F32(4.0 * F64(F32(sigma) * F32(sigma)))
    hyp = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    rt = [check_rt(R, tt, m, first, inl, K, n1, th2) for R, tt in hyp]
    g = [r[0] for r in rt]
    maxGood = max(g)
    nMinGood = max(int(0.9 * N), min_tri)
    nsimilar = sum(1 for x in g if x > 0.7 * maxGood)
    out = dict(ok=False, reason=3, n_good=g, N=N, parallax=F32(0), motions=hyp)
    if maxGood < nMinGood or nsimilar > 1:
        return out
    k = g.index(maxGood)  # the if / else if chain
    out.update(parallax=rt[k][3], reason=4, k=k)
    if rt[k][3] > min_parallax:
        out.update(ok=True, reason=0, R=hyp[k][0], t=hyp[k][1], P3D=rt[k][1], tri=rt[k][2])
    return out


def reconstruct_h(inl, H21, K, m, first, n1, sigma, min_parallax, min_tri):
    """ReconstructH (:572-733).  vP3D is never assigned (:724-730): no P3D in the result."""
    N = int(np.sum(inl))
    K = _f(K)
    A = (np.linalg.inv(K).astype(F32) @ _f(H21) @ K).astype(F32)
    U, w, Vt = np.linalg.svd(A)
    U, w, Vt = U.astype(F32), w.astype(F32), Vt.astype(F32)
    V = Vt.T
    s = F32(np.linalg.det(U)) * F32(np.linalg.det(Vt))
    d1, d2, d3 = w
    out = dict(ok=False, reason=2, n_good=[0] * 8, N=N, parallax=F32(0), motions=[])
    with np.errstate(all="ignore"):
        if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001:
            return out
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        hyp = []
        for i in range(4):
            Rp = np.zeros((3, 3), F32)
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = ct, -st[i], 1, st[i], ct
            R = (s * U @ Rp @ Vt).astype(F32)
            tp = _f([x1[i], 0, -x3[i]]) * (d1 - d3)
            t = (U @ tp).astype(F32)
            hyp.append((R, (t / F32(np.linalg.norm(t))).astype(F32)))
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        for i in range(4):
            Rp = np.zeros((3, 3), F32)
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
            R = (s * U @ Rp @ Vt).astype(F32)
            tp = _f([x1[i], 0, x3[i]]) * (d1 + d3)
            t = (U @ tp).astype(F32)
            hyp.append((R, (t / F32(np.linalg.norm(t))).astype(F32)))
    del V
    th2 = F32(4.0 * F64(F32(sigma) * F32(sigma)))
    bestGood, second, best, bestPar, bestTri, g = 0, 0, -1, F32(-1), None, []
    for i, (R, t) in enumerate(hyp):
        r = check_rt(R, t, m, first, inl, K, n1, th2)
        g.append(r[0])
        if r[0] > bestGood:
            second, bestGood, best, bestPar, bestTri = bestGood, r[0], i, r[3], r[2]
        elif r[0] > second:
            second = r[0]
    out.update(n_good=g, motions=hyp, reason=3, k=best)
    if second < 0.75 * bestGood and bestGood > min_tri and bestGood > 0.9 * N:
        out.update(reason=4, parallax=bestPar)
        if bestPar >= min_parallax:
            out.update(ok=True, reason=0, R=hyp[best][0], t=hyp[best][1], tri=bestTri)
    return out


def reconstruct(xy1, xy2, matches12, K, sets, sigma=1.0, rh_threshold=0.5, min_parallax=1.0, min_tri=50):
    """Reconstruct (:40-129): dict(ok, reason, model, SH, SF, H, F (the two searches), and the chosen model's result)"""
    xy1, xy2 = _f(xy1), _f(xy2)
    i1, i2 = matches_of(xy1, xy2, matches12)
    m = np.concatenate([xy1[i1], xy2[i2]], 1)
    H, F = find(0, xy1, xy2, i1, i2, sets, sigma), find(1, xy1, xy2, i1, i2, sets, sigma)
    bh, SH = first_maximum(H["score"])
    bf, SF = first_maximum(F["score"])
    out = dict(H=H, F=F, best_it_h=bh, best_it_f=bf, SH=SH, SF=SF, ok=False, model=1)
    if SH + SF == 0:
        out.update(reason=1)
        return out
    RH = SH / (SH + SF)
    out["RH"] = RH
    if RH > F32(rh_threshold):
        inl = H["inlier"][bh] if bh >= 0 else np.zeros(len(m), bool)
        out.update(model=0, **reconstruct_h(inl, H["M21"][bh], K, m, i1, len(xy1), sigma, F32(min_parallax), min_tri))
    else:
        inl = F["inlier"][bf] if bf >= 0 else np.zeros(len(m), bool)
        out.update(model=1, **reconstruct_f(inl, F["M21"][bf], K, m, i1, len(xy1), sigma, F32(min_parallax), min_tri))
    return out

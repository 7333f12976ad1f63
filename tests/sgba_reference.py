"""Optimizer::LocalBundleAdjustment WITH its planes and rooms restated in NumPy / Python float64: lba_reference.py (the visual
part) extended by the plane and room vertices and their edges, the stand-in for g2o in the tests of
vsg_mappoints_local_bundle_adjustment_sgraph as eg_reference.py is for the essential graph.

Written from the sources -- Optimizer.cc:2018-2232, :2342-2369, :2426-2441, OptimizableTypes.h:296-557, plane3d.h,
base_binary_edge.hpp:91-202, base_multi_edge.hpp:63-222, optimization_algorithm_levenberg.cpp -- independently of
csrc/vsg_sgraph_ba.h: atan2 / sin / cos are libm's (or `jit`, another libm whose results differ by 0 or +-1 ulp:
eg_reference.Jitter), every edge's quadratic form is a matrix product, the reduced system is ONE dense matrix over the
optimised keyframes, the planes with an edge and the rooms, filled by += per edge in edge order (`sem_order` permutes the
semantic edges, `order` the visual ones) and solved by lba_reference.ldlt_solve.  computeScale runs over the vertices in
g2o's order (poses, planes, rooms, then the marginalised points).

It logs how close every evaluation comes to a branch (Math.trace, the smallest over a run):
  seam   atan2's discontinuity: |y| / hypot where x < 0, else 1 (azimuth), the argument pairs of every azimuth();
  pole   elevation at +-pi/2: hypot(x, y) / |v| of every elevation() and azimuth() (where the azimuth is undefined);
  dir    |d| of every correctPlaneDirection (d == 0);
  fabs   | |d1| - |d2| | of every room branch;
  dist   |d| of the local plane in every isDistanceCorrect;
  chi2   |chi2 - threshold| / threshold of every compared chi2.
"""
import math
import struct

import numpy as np

import lba_reference as lr
from pose_reference import DBL_MAX, F32, oplus, q_mul

POINT_PLANE, PLANE_KF, ROOM2, ROOM4 = 0, 1, 2, 3
DELTA_1D, DELTA_3D = float(F32(math.sqrt(3.841))), float(F32(math.sqrt(7.815)))
TH_PK, TH_PP = 7.815, 3.841
NUM_DELTA = 1e-9


def scalar_jitter(seed):
    """eg_reference.Jitter on one Python float: 0 or +-1 ulp by a seeded hash of the result's bits; 0 and 1 stay."""
    s = (0x9E3779B97F4A7C15 * (2 * seed + 1)) & 0xFFFFFFFFFFFFFFFF
    M = 0xFFFFFFFFFFFFFFFF

    def jit(v):
        if not math.isfinite(v) or v == 0.0 or v == 1.0:
            return v
        z = (struct.unpack("<Q", struct.pack("<d", v))[0] + s) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        k = z % 3 - 1
        return math.nextafter(v, math.inf) if k > 0 else math.nextafter(v, -math.inf) if k < 0 else v
    return jit


class Math:
    def __init__(self, jit=None):
        self.jit = jit or (lambda v: v)
        self.trace = dict(seam=math.inf, pole=math.inf, dir=math.inf, fabs=math.inf, dist=math.inf, chi2=math.inf)

    def log(self, key, v):
        if math.isfinite(v):
            self.trace[key] = min(self.trace[key], v)

    def atan2(self, y, x):
        return self.jit(math.atan2(y, x))

    def sin(self, x):
        return self.jit(math.sin(x))

    def cos(self, x):
        return self.jit(math.cos(x))

    def azimuth(self, v):
        h, n = math.hypot(v[0], v[1]), math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        self.log("seam", abs(v[1]) / h if v[0] < 0 and h > 0 else 1.0)
        self.log("pole", h / n if n > 0 else 0.0)
        return self.atan2(v[1], v[0])

    def elevation(self, v):
        return self.atan2(v[2], math.sqrt(v[0] * v[0] + v[1] * v[1]))


def q_matrix(q):
    """Eigen's toRotationMatrix, x y z w."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def normalize(c):
    c = np.asarray(c, np.float64)
    return c * (1. / math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]))


def rotation(m, v):
    """Plane3D::rotation: AngleAxis(az, Z) * AngleAxis(-el, Y) as Eigen multiplies them, as quaternions."""
    az, el = m.azimuth(v), m.elevation(v)
    qz = np.array([0.0, 0.0, m.sin(0.5 * az), m.cos(0.5 * az)])
    qy = np.array([0.0, m.sin(0.5 * -el), 0.0, m.cos(0.5 * -el)])
    return q_matrix(q_mul(qz, qy))


def plane_oplus(m, c, v):
    s, cc = m.sin(v[1]), m.cos(v[1])
    n = np.array([cc * m.cos(v[0]), cc * m.sin(v[0]), s])
    R = rotation(m, c[:3])
    d = -c[3] + v[2]
    return normalize(np.concatenate([R @ n, [-d]]))


def plane_ominus(m, a, b):
    n = rotation(m, a[:3]).T @ b[:3]
    return np.array([m.azimuth(n), m.elevation(n), -a[3] - -b[3]])


def plane_transform(est, c):
    R = q_matrix(est[0])
    n = R @ c[:3]
    return normalize(np.concatenate([n, [c[3] - est[1] @ n]]))


def point_plane_error(est, Pj, G):
    qi = np.array([-est[0][0], -est[0][1], -est[0][2], est[0][3]])
    Ti = np.eye(4)
    Ti[:3, :3] = q_matrix(qi)
    Ti[:3, 3] = Ti[:3, :3] @ (est[1] * -1.)
    return np.array([((Pj @ Ti) @ G) @ Ti.T @ Pj])


def wall_pair(m, w1, w2):
    a, b = np.array(w1, np.float64), np.array(w2, np.float64)
    m.log("dir", abs(a[3])), m.log("dir", abs(b[3]))
    if a[3] > 0:
        a = a * -1
    if b[3] > 0:
        b = b * -1
    da, db = abs(a[3]), abs(b[3])
    m.log("fabs", abs(da - db))
    if da > db:
        return (0.5 * (da * a[:3] - db * b[:3])) + db * b[:3]
    return (0.5 * (db * b[:3] - da * a[:3])) + da * a[:3]


class SGraph(lr.Graph):
    """lba_reference.Graph with the semantic vertices and edges of a scene's `sem` dict (sgba_scenes.py)."""

    def __init__(self, s, order=None, sem_order=None, jit=None):
        super().__init__(s, order)
        q = s["sem"]
        self.m = Math(jit)
        self.plane0 = np.asarray(q["plane_eq"], np.float64).reshape(-1, 4)
        self.Pl = len(self.plane0)
        off = np.asarray(q["pl_obs_off"], np.int64)
        self.o_pl = np.repeat(np.arange(self.Pl), np.diff(off))
        self.o_kf = np.asarray(q["pl_obs_kf"], np.int64)[:len(self.o_pl)]
        self.NO = len(self.o_pl)
        self.local = np.asarray(q["pl_obs_local"], np.float64).reshape(-1, 4)
        self.G = np.asarray(q["pl_obs_G"], np.float64).reshape(-1, 4, 4)
        wk, wp = np.asarray(q["w_plane_kf"], np.float64), np.asarray(q["w_plane_point"], np.float64)
        self.room0 = np.asarray(q["room_center"], np.float64).reshape(-1, 3)
        self.R = len(self.room0)
        walls, nw = np.asarray(q["room_wall"], np.int64).reshape(-1, 4), np.asarray(q["room_n_walls"], np.int64)
        # the edges, in g2o's insertion order: (kind, vertex 0, observation, planes, information)
        self.edges, self.o_pk, self.o_pp = [], np.full(self.NO, -1), np.full(self.NO, -1)
        for o in range(self.NO):
            if wk[o] > 0:
                self.o_pk[o] = len(self.edges)
                self.edges.append((PLANE_KF, int(self.o_kf[o]), o, [int(self.o_pl[o])], float(wk[o])))
            if wp[o] > 0:
                self.o_pp[o] = len(self.edges)
                self.edges.append((POINT_PLANE, int(self.o_kf[o]), o, [int(self.o_pl[o])], float(wp[o])))
        self.n_plane_edges = len(self.edges)
        for r in range(self.R):
            self.edges.append((ROOM4 if nw[r] == 4 else ROOM2, r, -1, [int(w) for w in walls[r, :nw[r]]], 1.0))
        self.Es = len(self.edges)
        self.sem_order = list(range(self.Es)) if sem_order is None else [int(e) for e in sem_order]
        # a keyframe with a plane edge is a vertex too: the optimised keyframes and the Schur pairs again
        has = np.bincount(self.kf, minlength=self.K) > 0
        for kind, v0, *_ in self.edges[:self.n_plane_edges]:
            has[v0] = True
        self.opt_kf = np.flatnonzero(~self.fixed & has)
        self.Ko = len(self.opt_kf)
        self.opt_of = np.full(self.K, -1)
        self.opt_of[self.opt_kf] = np.arange(self.Ko)
        self.eo = self.opt_of[self.kf]
        pa, pb = [], []
        for p in range(self.P):
            es = [e for e in range(np.asarray(s["obs_off"])[p], np.asarray(s["obs_off"])[p + 1]) if self.eo[e] >= 0]
            for a in es:
                for b in es:
                    pa.append(a), pb.append(b)
        self.pa, self.pb = np.array(pa, np.int64), np.array(pb, np.int64)
        used = np.zeros(self.Pl, bool)
        for e in self.edges:
            used[e[3]] = True
        self.act_planes = np.flatnonzero(used)
        self.Pa = len(self.act_planes)
        self.pl_row = np.full(self.Pl, -1)
        self.pl_row[self.act_planes] = 6 * self.Ko + 3 * np.arange(self.Pa)
        self.rm_row = 6 * self.Ko + 3 * self.Pa + 6 * np.arange(self.R)
        self.n = 6 * self.Ko + 3 * self.Pa + 6 * self.R
        self.sem_chi2 = np.zeros(self.Es)

    def sem_error(self, edge, v0, planes):
        kind, _, o, _, _ = edge
        if kind == POINT_PLANE:
            return point_plane_error(v0, planes[0], self.G[o])
        if kind == PLANE_KF:
            return plane_ominus(self.m, plane_transform(v0, planes[0]), self.local[o])
        vec = wall_pair(self.m, planes[0], planes[1])
        if kind == ROOM4:
            vec = vec + wall_pair(self.m, planes[2], planes[3])
        return v0[1] - vec

    def vertices(self, edge, est, pl, rm):
        kind, v0, _, ps, _ = edge
        return (est[v0] if kind <= PLANE_KF else rm[v0]), [pl[p] for p in ps]

    def sem_delta(self, edge):
        return DELTA_1D if edge[0] == POINT_PLANE else DELTA_3D

    def sem_robust(self, edge, chi2):
        d = self.sem_delta(edge)
        if chi2 <= d * d:
            return chi2, 1.0
        sq = math.sqrt(chi2)
        return 2 * sq * d - d * d, d / sq

    def sem_chi(self, est, pl, rm):
        """computeActiveErrors + activeRobustChi2 of the semantic edges, serial in sem_order."""
        cost = np.zeros(self.Es)
        for e, edge in enumerate(self.edges):
            v0, ps = self.vertices(edge, est, pl, rm)
            err = self.sem_error(edge, v0, ps)
            self.sem_chi2[e] = float(err @ (edge[4] * err))
            cost[e] = self.sem_robust(edge, self.sem_chi2[e])[0]
        c = cost[self.sem_order]
        return float(np.cumsum(c)[-1]) if len(c) else 0.0

    def sem_build(self, est, pl, rm):
        """linearizeOplus (numeric) and constructQuadraticForm of the semantic edges into H (n, n) and b (n)."""
        n = self.n
        self.Hs_sem, self.b_sem = np.zeros((n, n)), np.zeros(n)
        cost = np.zeros(self.Es)
        scalar = 1.0 / (2 * NUM_DELTA)
        for e in self.sem_order:
            edge = self.edges[e]
            kind, i0, _, ps, w = edge
            v0, planes = self.vertices(edge, est, pl, rm)
            err = self.sem_error(edge, v0, planes)
            cols = 6 + 3 * len(ps)
            J, rows = np.zeros((len(err), cols)), np.full(cols, -1)
            first = self.rm_row[i0] if kind >= ROOM2 else (6 * self.opt_of[i0] if self.opt_of[i0] >= 0 else -1)
            if first >= 0:
                rows[:6] = first + np.arange(6)
                for d in range(6):
                    u = np.zeros(6)
                    u[d] = NUM_DELTA
                    ep = self.sem_error(edge, oplus(v0, u), planes)
                    u[d] = -NUM_DELTA
                    J[:, d] = scalar * (ep - self.sem_error(edge, oplus(v0, u), planes))
            for k, p in enumerate(ps):
                rows[6 + 3 * k:9 + 3 * k] = self.pl_row[p] + np.arange(3)
                for d in range(3):
                    u = np.zeros(3)
                    u[d] = NUM_DELTA
                    ep = self.sem_error(edge, v0, planes[:k] + [plane_oplus(self.m, planes[k], u)] + planes[k + 1:])
                    u[d] = -NUM_DELTA
                    em = self.sem_error(edge, v0, planes[:k] + [plane_oplus(self.m, planes[k], u)] + planes[k + 1:])
                    J[:, 6 + 3 * k + d] = scalar * (ep - em)
            chi2 = float(err @ (w * err))
            self.sem_chi2[e] = chi2
            cost[e], rho1 = self.sem_robust(edge, chi2)
            live = rows >= 0
            Jl, rl = J[:, live], rows[live]
            self.Hs_sem[np.ix_(rl, rl)] += Jl.T @ (rho1 * w * np.eye(len(err))) @ Jl
            self.b_sem[rl] += Jl.T @ (-(w * err) * rho1)
        c = cost[self.sem_order]
        return float(np.cumsum(c)[-1]) if len(c) else 0.0

    def reduced(self, lam):
        """lba_reference.Graph.solve up to the reduced system of the keyframes -> Hs (6 Ko, 6 Ko) with lambda, bs, Dinv."""
        Ko, eo = self.Ko, self.eo
        Hll = self.Hll + lam * np.eye(3)
        Hll[~self.vertex_pt] = np.eye(3)
        Dinv = np.linalg.inv(Hll)
        W = self.Hpl @ Dinv[self.pt]
        Hs = np.zeros((Ko, Ko, 6, 6))
        Hs[np.arange(Ko), np.arange(Ko)] = self.Hpp + lam * np.eye(6)
        if len(self.pa):
            np.subtract.at(Hs, (eo[self.pa], eo[self.pb]), W[self.pa] @ self.Hpl[self.pb].transpose(0, 2, 1))
        bs = self.bp.copy()
        oo = self.order[eo[self.order] >= 0]
        np.subtract.at(bs, eo[oo], (W @ self.bl[self.pt][:, :, None])[oo, :, 0])
        return Hs.transpose(0, 2, 1, 3).reshape(6 * Ko, 6 * Ko), bs.reshape(-1), Dinv

    def backsub(self, Dinv, xp):
        eo = self.eo
        oo = self.order[eo[self.order] >= 0]
        r = self.bl.copy()
        np.subtract.at(r, self.pt[oo], (self.Hpl.transpose(0, 2, 1)[oo] @ xp[eo[oo]][:, :, None])[:, :, 0])
        xl = (Dinv @ r[:, :, None])[:, :, 0]
        xl[~self.vertex_pt] = 0.0
        return xl


def local_ba_sgraph(s, order=None, sem_order=None, jit=None, stop_flag=False):
    """-> lba_reference.local_ba's dict plus plane_out (Pl, 4), room_out (R, 3), erase_plane, chi2_pk, chi2_pp (NaN where the
    edge does not exist), the semantic counters, `branch` (Math.trace) and `trace` (the Levenberg decisions)."""
    K, P = len(s["kfs"]), len(s["slots"])
    q = s["sem"]
    Tin = np.asarray(s["Tcw"], F32).reshape(K, 7)
    pos_in = np.asarray(s["store_pos"], F32)[np.asarray(s["slots"], np.int64)].reshape(P, 3)
    fixed = np.asarray(s["fixed"]).astype(bool)
    E = int(np.asarray(s["obs_off"])[-1]) if P else 0
    plane0 = np.asarray(q["plane_eq"], np.float64).reshape(-1, 4)
    room0 = np.asarray(q["room_center"], np.float64).reshape(-1, 3)
    NO = int(np.asarray(q["pl_obs_off"])[-1])
    n_pk = int((np.asarray(q["w_plane_kf"], np.float64)[:NO] > 0).sum())
    n_pp = int((np.asarray(q["w_plane_point"], np.float64)[:NO] > 0).sum())
    out = dict(ran=0, kf_out=Tin.astype(np.float64), pos_out=pos_in.copy(), erase=np.zeros(E, np.uint8), chi2=np.zeros(E),
               n_opt_kf=int((~fixed).sum()) if P else 0, n_fixed_kf=int(fixed.sum()) if P else 0, n_points=P, n_edges=E, trace=[],
               plane_out=plane0.copy(), room_out=room0.copy(), erase_plane=np.zeros(NO, np.uint8), chi2_pk=np.full(NO, np.nan),
               chi2_pp=np.full(NO, np.nan))
    if P == 0 or not fixed.any() or E + n_pk + n_pp == 0 or stop_flag:  # :1734, :2277 (no room edge counted), :2283
        return out
    g = SGraph(s, order, sem_order, jit)
    est, X = list(g.est), g.X.copy()
    pl = [g.plane0[i].copy() for i in range(g.Pl)]
    rm = [(np.array([0.0, 0.0, 0.0, 1.0]), g.room0[r].copy()) for r in range(g.R)]
    lam = ni = 0.0
    n_bad = its = trials = 0
    stop, chi_initial, current = lr.STOP_ITERATIONS, 0.0, 0.0
    nk, n = 6 * g.Ko, g.n
    with np.errstate(all="ignore"):
        for it in range(s["iterations"]):
            current = g.build(est, X) + g.sem_build(est, pl, rm)
            ini = current
            Hkk = g.Hs_sem[:nk, :nk]
            for i in range(g.Ko):  # the keyframes' semantic blocks belong to Hpp / bp
                g.Hpp[i] += Hkk[6 * i:6 * i + 6, 6 * i:6 * i + 6]
                g.bp[i] += g.b_sem[6 * i:6 * i + 6]
            if it == 0:
                d = np.concatenate([np.abs(np.einsum("kii->ki", g.Hpp)).ravel(), np.abs(np.diag(g.Hs_sem)[nk:]),
                                    np.abs(np.einsum("pii->pi", g.Hll))[g.vertex_pt].ravel()])
                lam, ni, n_bad, chi_initial = 1e-5 * float(np.max(d)), 2.0, 0, current
            rho, qmax, tr = 0.0, 0, []
            while True:
                Hs, bs, Dinv = g.reduced(lam)
                A = g.Hs_sem.copy()
                A[:nk, :nk] = Hs
                A[np.arange(nk, n), np.arange(nk, n)] += lam
                b = g.b_sem.copy()
                b[:nk] = bs
                ok2, x = lr.ldlt_solve(A, b)
                xp = x[:nk].reshape(g.Ko, 6)
                xl = g.backsub(Dinv, xp)
                cand = list(est)
                for i, k in enumerate(g.opt_kf):
                    cand[k] = oplus(est[k], xp[i])
                cpl = list(pl)
                for p in g.act_planes:
                    cpl[p] = plane_oplus(g.m, pl[p], x[g.pl_row[p]:g.pl_row[p] + 3])
                crm = [oplus(rm[r], x[g.rm_row[r]:g.rm_row[r] + 6]) for r in range(g.R)]
                Xc = X + xl
                temp = g.chi(cand, Xc) + g.sem_chi(cand, cpl, crm)
                if not ok2:
                    temp = DBL_MAX
                xs = np.concatenate([x, xl[g.vertex_pt].ravel()])
                bsv = np.concatenate([g.bp.ravel(), g.b_sem[nk:], g.bl[g.vertex_pt].ravel()])
                sc = xs * (lam * xs + bsv)
                scale = (float(np.cumsum(sc)[-1]) if len(sc) else 0.0) + 1e-3
                rho = (current - temp) / scale
                good = bool(rho > 0 and np.isfinite(temp))
                if good:
                    alpha = min(1. - float(np.float64(2 * rho - 1) ** 3), 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni, current, est, X, pl, rm = 2.0, temp, cand, Xc, cpl, crm
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
                stop = lr.STOP_TERMINATE
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                stop = lr.STOP_BAD
                break
        Xcam, _ = g.camera_points(est, X)
        depth_positive = Xcam[:, 2] > 0.0 if E else np.zeros(0, bool)
        th = np.where(g.stereo, lr.TH[1], lr.TH[0])
        out["erase"] = ((g.chi2 > th) | ~depth_positive).astype(np.uint8)
        for c, t in zip(g.chi2, th):
            g.m.log("chi2", abs(c - t) / t)
        for o in range(g.NO):
            d = plane_transform(est[g.o_kf[o]], pl[g.o_pl[o]])[3]
            g.m.log("dist", abs(d))
            flag = False
            for e, t, key in ((g.o_pk[o], TH_PK, "chi2_pk"), (g.o_pp[o], TH_PP, "chi2_pp")):
                if e >= 0:
                    out[key][o] = g.sem_chi2[e]
                    g.m.log("chi2", abs(g.sem_chi2[e] - t) / t)
                    flag = flag or g.sem_chi2[e] > t or not d > 0
            out["erase_plane"][o] = flag
    out["chi2"] = g.chi2.copy()
    for k in g.opt_kf:
        out["kf_out"][k] = np.concatenate(est[k])
    out["pos_out"][g.vertex_pt] = X[g.vertex_pt].astype(F32)
    for p in g.act_planes:
        out["plane_out"][p] = pl[p]
    for r in range(g.R):
        out["room_out"][r] = rm[r][1]
    out.update(ran=1, n_mono=int((~g.stereo).sum()), n_stereo=int(g.stereo.sum()), n_erase=int(out["erase"].sum()),
               iterations_run=its, trials_run=trials, stop_reason=stop, **{"lambda": lam}, chi2_initial=chi_initial,
               chi2_final=current, n_planes_active=g.Pa, n_rooms_active=g.R, n_plane_kf=n_pk, n_plane_point=n_pp, n_room_edges=g.R,
               n_rows=g.n, n_erase_plane=int(out["erase_plane"].sum()), branch=dict(g.m.trace))
    return out

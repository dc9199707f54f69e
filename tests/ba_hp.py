"""The first Levenberg-Marquardt trial of Bundle::Compute (jni/Bundle.cc:136-178, the first pass of Do_LM_Step :202-501) restated
in extended precision (numpy longdouble), WITHOUT the Schur complement: the full damped normal matrix of every adjustable camera
and every point is built and solved by dense Gaussian elimination with partial pivoting.  It is the yardstick of the fast
summation mode: a device result is held to "no further from this than the sequential fp64 sum of the oracle".

The expressions are the reference's (ATAN camera with its derivative rule, the Tukey weight 1 - e^2 / sigma^2 of
MEstimator.h, generator fields, the exponential map of RT.h with its small-angle branches); only the arithmetic is wider.  The
constants of the algorithm (camera parameters, Tukey and MAD factors, sigma floor, lambda) are the fp64 values the program uses.
Measurement lists with a duplicated (camera, point) pair are not supported (the reference's reduced system sees only the last).
"""
import numpy as np

LD = np.longdouble


class Camera:
    """jni/ATANCamera.{h,cc}: Project and GetProjectionDerivs_Eigen, in longdouble."""

    def __init__(self, cam5, w, h):
        p = [LD(x) for x in cam5]
        self.focal = (LD(w) * p[0], LD(h) * p[1])
        self.center = (LD(w) * p[2] - LD(0.5), LD(h) * p[3] - LD(0.5))
        self.w = p[4]
        self.enabled = self.w != 0
        self.two_tan = LD(2) * np.tan(self.w / LD(2)) if self.enabled else LD(0)
        self.winv = LD(1) / self.w if self.enabled else LD(0)

    def project(self, x, y):
        r = np.sqrt(x * x + y * y)
        factor = LD(1) if (r < 0.001 or not self.enabled) else self.winv * np.arctan(r * self.two_tan) / r
        im = (self.center[0] + self.focal[0] * (x * factor), self.center[1] + self.focal[1] * (y * factor))
        return im, r, factor

    def derivs(self, x, y, r, factor):
        k = self.two_tan
        rr = r if self.enabled else LD(0)
        if rr < 0.01:
            dx = dy = LD(0)
        else:
            dx = self.winv * (k * x) / (rr * rr * (1 + k * k * rr * rr)) - x * factor / (rr * rr)
            dy = self.winv * (k * y) / (rr * rr * (1 + k * k * rr * rr)) - y * factor / (rr * rr)
        return np.array([self.focal[0] * (dx * x + factor), self.focal[0] * (dy * x),
                         self.focal[1] * (dx * y), self.focal[1] * (dy * y + factor)], dtype=LD)


def se3_exp(mu):
    """jni/RT.h:318-352 mySE3::exp with its branches; mu = (translation, rotation).  -> (R 3x3, t 3)"""
    mu = np.asarray(mu, dtype=LD)
    U, W = mu[:3], mu[3:]
    theta_sq = W @ W
    theta = np.sqrt(theta_sq)
    cr = np.cross(W, U)
    one_6th, one_20th = LD(1) / 6, LD(1) / 20
    if theta_sq < 1e-8:
        A, B = 1 - one_6th * theta_sq, LD(0.5)
        t = U + LD(0.5) * cr
    else:
        if theta_sq < 1e-6:
            C = one_6th * (1 - one_20th * theta_sq)
            A, B = 1 - theta_sq * C, LD(0.5) - LD(0.25) * one_6th * theta_sq
        else:
            A = np.sin(theta) / theta
            B = (1 - np.cos(theta)) / theta_sq
            C = (1 - A) / theta_sq
        t = U + B * cr + C * np.cross(W, cr)
    K = np.array([[0, -W[2], W[1]], [W[2], 0, -W[0]], [-W[1], W[0], 0]], dtype=LD)
    R = np.eye(3, dtype=LD) + A * K + B * (K @ K)
    return R, t


def solve_dense(H, g):
    """H x = g by Gaussian elimination with partial pivoting (first row of largest |pivot|), all in longdouble."""
    A = np.array(H, dtype=LD)
    b = np.array(g, dtype=LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if A[p, k] == 0:
            raise np.linalg.LinAlgError("singular")
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def tukey_sigma2(e2, min_sigma=0.4):
    """find_sigma_squared(EST_TUKEY) of MEstimator.h (median = element n/2 of the sorted list), clamped at min_sigma^2 (:224-227)."""
    v = np.sort(np.asarray(e2, dtype=LD))
    n = len(v)
    med = v[n // 2]
    sigma = LD(1.4826) * (1 + LD(5.0) / LD(n * 2 - 6)) * np.sqrt(med)
    sigma = LD(4.6851) * sigma
    s2 = sigma * sigma
    lo = LD(min_sigma) * LD(min_sigma)
    return s2 if s2 >= lo else lo


def first_trial(cam5, w, h, cams, fixed, pts, meas, lam=1e-4, min_sigma=0.4):
    """cams [n][12] (R row-major, t), fixed [n], pts [m][3], meas [(cam, point, (x, y), sigma^2)] in AddMeas order.
    -> dict: cams, pts (the trial state, longdouble), sigma2, cur_err (dCurrentError), new_err (FindNewError at the trial),
    n_free, n_unknowns."""
    cam = Camera(cam5, w, h)
    cams = np.asarray(cams, dtype=LD)
    pts = np.asarray(pts, dtype=LD)
    nc, npt = len(cams), len(pts)
    Rs = [cams[j, :9].reshape(3, 3) for j in range(nc)]
    ts = [cams[j, 9:] for j in range(nc)]
    row = {}
    for j in range(nc):
        if not fixed[j]:
            row[j] = 6 * len(row)
    nS = 6 * len(row)

    def residual(R, t, X, found, sin):
        c = R @ X + t
        if c[2] <= 0:
            return None
        x, y = c[0] / c[2], c[1] / c[2]
        im, r, factor = cam.project(x, y)
        e = np.array([(LD(found[0]) - im[0]) * sin, (LD(found[1]) - im[1]) * sin], dtype=LD)
        return c, x, y, r, factor, e

    # pass 1 (:209-215): squared errors, median, sigma^2
    res = []
    for (j, i, found, s2) in meas:
        sin = np.sqrt(LD(1) / LD(s2))
        res.append((residual(Rs[j], ts[j], pts[i], found, sin), sin))
    e2 = [r[0][5] @ r[0][5] for r in res if r[0] is not None]
    sigma2 = tukey_sigma2(e2, min_sigma)

    # pass 2 (:241-321): weights, Jacobians, the full normal matrix (cameras first, then points)
    n = nS + 3 * npt
    H = np.zeros((n, n), dtype=LD)
    g = np.zeros(n, dtype=LD)
    cur = LD(0)
    for (j, i, found, s2), (r, sin) in zip(meas, res):
        if r is None:
            cur += 1
            continue
        c, x, y, rad, factor, e = r
        err2 = e @ e
        wt = LD(0) if err2 > sigma2 else 1 - err2 / sigma2
        if wt == 0:
            cur += 1
            continue
        d = wt * cam.derivs(x, y, rad, factor)
        D = (sin * d).reshape(2, 2)
        eps = wt * e
        cur += 1 - (1 - err2 / sigma2) ** 3
        ooz = 1 / c[2]

        def dproj(mot):                                       # d(projection)/d(motion of the camera-frame point)
            return D @ np.array([(mot[0] - c[0] * mot[2] * ooz) * ooz, (mot[1] - c[1] * mot[2] * ooz) * ooz], dtype=LD)

        B = np.stack([dproj(Rs[j][:, k]) for k in range(3)], 1)            # 2 x 3
        pr = nS + 3 * i
        H[pr:pr + 3, pr:pr + 3] += B.T @ B
        g[pr:pr + 3] += B.T @ eps
        if j in row:
            v4 = (c[0], c[1], c[2], LD(1))
            gens = []
            for k in range(6):                                # generator_field(k, (x, y, z, 1)), jni/RT.h:297-308
                mot = [LD(0)] * 3
                if k < 3:
                    mot[k] = v4[3]
                else:
                    mot[(k + 1) % 3] = -v4[(k + 2) % 3]
                    mot[(k + 2) % 3] = v4[(k + 1) % 3]
                gens.append(dproj(mot))
            A = np.stack(gens, 1)                             # 2 x 6
            cr = row[j]
            H[cr:cr + 6, cr:cr + 6] += A.T @ A
            g[cr:cr + 6] += A.T @ eps
            Wm = A.T @ B
            H[cr:cr + 6, pr:pr + 3] += Wm
            H[pr:pr + 3, cr:cr + 6] += Wm.T

    # LM damping of the diagonal (:329-347 V*, :370 U*); a point whose V has a zero diagonal element has V*^-1 = 0 in the
    # reference: it takes no part in the step, so its rows and columns are left out of the system here
    keep = np.ones(n, bool)
    for i in range(npt):
        pr = nS + 3 * i
        if H[pr, pr] * H[pr + 1, pr + 1] * H[pr + 2, pr + 2] == 0:
            keep[pr:pr + 3] = False
    idx = np.nonzero(keep)[0]
    Hk = H[np.ix_(idx, idx)]
    Hk[np.diag_indices(len(idx))] *= 1 + LD(lam)
    delta = np.zeros(n, dtype=LD)
    delta[idx] = solve_dense(Hk, g[idx])

    # the trial state (:476-485): pose_new = exp(camera update) * pose, pos_new = pos + map update
    out_c = np.array(cams, dtype=LD)
    for j, cr in row.items():
        Re, te = se3_exp(delta[cr:cr + 6])
        out_c[j, :9] = (Re @ Rs[j]).ravel()
        out_c[j, 9:] = Re @ ts[j] + te
    out_p = pts + delta[nS:].reshape(npt, 3)

    # FindNewError (:537-561) at the trial state
    ne = LD(0)
    for (j, i, found, s2) in meas:
        r = residual(out_c[j, :9].reshape(3, 3), out_c[j, 9:], out_p[i], found, np.sqrt(LD(1) / LD(s2)))
        if r is None:
            ne += 1
            continue
        e2n = r[5] @ r[5]
        ne += 1 if e2n > sigma2 else 1 - (1 - e2n / sigma2) ** 3
    return {"cams": out_c, "pts": out_p, "sigma2": sigma2, "cur_err": cur, "new_err": ne, "n_free": len(row), "n_unknowns": len(idx)}


def bar(gpu, oracle, hp):
    """The fast mode's bar against the extended-precision trial: max|gpu - hp| <= 8 max|oracle - hp| + 16 eps max|hp|.
    -> (gpu error, allowed, oracle error), all as float."""
    hp64 = np.asarray(hp, dtype=LD)
    dg = float(np.abs(np.asarray(gpu, dtype=LD) - hp64).max())
    do = float(np.abs(np.asarray(oracle, dtype=LD) - hp64).max())
    scale = float(np.abs(hp64).max())
    return dg, 8 * do + 16 * np.finfo(np.float64).eps * scale, do

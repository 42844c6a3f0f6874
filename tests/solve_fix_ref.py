"""Kernel-order restatement of k_solve_plane and k_solve_fix (radio-mapper_amd/csrc/solve_path.hpp), an independent
numpy.linalg statement of the same quantities, and the scenes and the Monte-Carlo helper of the solve_fix tests.  TEST
INFRASTRUCTURE ONLY.

The restatement follows tests/solve_kernel_ref.py: float64, the kernels' order of sums and products, one rounding per
operation, every pair's terms elementwise over pairs and windows, every sum over the pairs a Python loop in list order
(_seq_sum).  Only + - * / and np.sqrt touch the values; np.isfinite and np.where select, they do not round.  The NaN path
is part of the contract, so everything runs under np.errstate(all="ignore")."""
import numpy as np

import solve_kernel_ref as kr
from solve_kernel_ref import _f_at, _seq_sum

SINGULAR = 1e-12        # kSolveSingular


def as_plane(origin, e1, e2):
    return np.concatenate([np.asarray(origin, np.float64), np.asarray(e1, np.float64), np.asarray(e2, np.float64)])


def _inputs(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample):
    buoys = np.ascontiguousarray(buoy_xyz, dtype=np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    li = np.asarray(lag_int, dtype=np.int32)
    lf = np.asarray(lag_frac, dtype=np.float32)
    W, P = li.shape
    assert lf.shape == (W, P) and len(pairs) == P
    wg = None if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
    assert wg is None or wg.shape == (W, P)
    mps = np.float64(metres_per_sample)
    with np.errstate(all="ignore"):
        d = np.ascontiguousarray(((li.astype(np.float64) + lf.astype(np.float64)) * mps).T)      # [P][W]
    wg = 1.0 if wg is None else np.ascontiguousarray(wg.T)
    return buoys, buoys[pairs[:, 0]], buoys[pairs[:, 1]], d, wg, W


def _point(o, e1, e2, u1, u2):
    """p(u) = o + u1 e1 + u2 e2, each coordinate summed left to right"""
    return (o[0] + u1 * e1[0] + u2 * e2[0], o[1] + u1 * e1[1] + u2 * e2[1], o[2] + u1 * e1[2] + u2 * e2[2])


def _rows(x, y, z, b1, b2, d):
    """the pair loop's head: r [P][n] and the Jacobian entries jx, jy, jz [P][n] at (x, y, z)"""
    v1x, v1y, v1z = x - b1[:, 0, None], y - b1[:, 1, None], z - b1[:, 2, None]
    v2x, v2y, v2z = x - b2[:, 0, None], y - b2[:, 1, None], z - b2[:, 2, None]
    n1 = np.sqrt(v1x * v1x + v1y * v1y + v1z * v1z)
    n2 = np.sqrt(v2x * v2x + v2y * v2y + v2z * v2z)
    r = n2 - n1 - d
    return r, v2x / n2 - v1x / n1, v2y / n2 - v1y / n1, v2z / n2 - v1z / n1


def plane_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, plane, max_iter=60):
    """k_solve_plane.  plane: 9 floats (o, e1, e2).  Returns (pos float64 [W][3], cost float64 [W], iters int32 [W])."""
    buoys, b1, b2, d_all, wg_all, W = _inputs(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample)
    assert max_iter >= 1
    pl = np.asarray(plane, np.float64).reshape(9)
    o, e1, e2 = pl[0:3], pl[3:6], pl[6:9]
    n_buoys = len(buoys)
    with np.errstate(all="ignore"):
        cx = cy = cz = np.float64(0.0)
        for b in range(n_buoys):
            cx = cx + buoys[b, 0]
            cy = cy + buoys[b, 1]
            cz = cz + buoys[b, 2]
        cx, cy, cz = cx / np.float64(n_buoys), cy / np.float64(n_buoys), cz / np.float64(n_buoys)
        s1 = (cx - o[0]) * e1[0] + (cy - o[1]) * e1[1] + (cz - o[2]) * e1[2]
        s2 = (cx - o[0]) * e2[0] + (cy - o[1]) * e2[1] + (cz - o[2]) * e2[2]
        sx, sy, sz = _point(o, e1, e2, s1, s2)
        u1, u2 = np.full(W, s1), np.full(W, s2)
        px, py, pz = np.full(W, sx), np.full(W, sy), np.full(W, sz)
        lam = np.full(W, 1e-3)
        f = _f_at(px, py, pz, b1, b2, d_all, wg_all)
        it = np.zeros(W, np.int32)
        act = np.arange(W)
        while act.size:
            it[act] += 1
            x, y, z, a1, a2, lm, fa = px[act], py[act], pz[act], u1[act], u2[act], lam[act], f[act]
            d = d_all[:, act]
            ww = wg_all if np.ndim(wg_all) == 0 else wg_all[:, act]
            r, jx, jy, jz = _rows(x, y, z, b1, b2, d)
            j1 = jx * e1[0] + jy * e1[1] + jz * e1[2]
            j2 = jx * e2[0] + jy * e2[1] + jz * e2[2]
            a00, a01, a11, g0, g1 = _seq_sum(np.stack([ww * j1 * j1, ww * j1 * j2, ww * j2 * j2, ww * j1 * r, ww * j2 * r],
                                                      axis=1))
            d00, d11 = a00 * (1.0 + lm), a11 * (1.0 + lm)
            ok = d00 > 0.0
            l00 = np.sqrt(np.where(ok, d00, 1.0))
            l10 = a01 / l00
            t11 = d11 - l10 * l10
            ok = ok & (t11 > 0.0)
            l11 = np.sqrt(np.where(ok, t11, 1.0))
            y0 = -g0 / l00
            y1 = (-g1 - l10 * y0) / l11
            d2 = y1 / l11
            d1 = (y0 - l10 * d2) / l00
            t1, t2 = a1 + d1, a2 + d2
            tx, ty, tz = _point(o, e1, e2, t1, t2)
            fn = _f_at(tx, ty, tz, b1, b2, d, ww)
            acc = ok & (fn < fa)
            dn = np.sqrt(d1 * d1 + d2 * d2)
            u1[act], u2[act] = np.where(acc, t1, a1), np.where(acc, t2, a2)
            px[act], py[act], pz[act] = np.where(acc, tx, x), np.where(acc, ty, y), np.where(acc, tz, z)
            f[act] = np.where(acc, fn, fa)
            third = lm / 3.0
            lm_new = np.where(acc, np.where(third > 1e-12, third, 1e-12), lm * 4.0)
            lam[act] = lm_new
            stop = np.where(acc, dn < 1e-4, lm_new > 1e12) | (it[act] >= max_iter)
            act = act[~stop]
    return np.stack([px, py, pz], axis=1), f, it


def fix_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, pos, plane=None):
    """k_solve_fix<plane given> at pos [W][3].  Returns (info, cov float64 [W][3 or 6], resid float64 [W][P])."""
    buoys, b1, b2, d, ww, W = _inputs(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample)
    pos = np.asarray(pos, np.float64).reshape(W, 3)
    inf = np.float64(np.inf)
    with np.errstate(all="ignore"):
        r, jx, jy, jz = _rows(pos[:, 0], pos[:, 1], pos[:, 2], b1, b2, d)
        if plane is not None:
            pl = np.asarray(plane, np.float64).reshape(9)
            e1, e2 = pl[3:6], pl[6:9]
            j1 = jx * e1[0] + jy * e1[1] + jz * e1[2]
            j2 = jx * e2[0] + jy * e2[1] + jz * e2[2]
            a00, a01, a11 = _seq_sum(np.stack([ww * j1 * j1, ww * j1 * j2, ww * j2 * j2], axis=1))
            fin = np.isfinite(a00) & np.isfinite(a01) & np.isfinite(a11)
            ok = fin & (a00 > SINGULAR * a00)
            l00 = np.sqrt(np.where(ok, a00, 1.0))
            l10 = a01 / l00
            t11 = a11 - l10 * l10
            ok = ok & (t11 > SINGULAR * a11) & np.isfinite(t11)
            l11 = np.sqrt(np.where(ok, t11, 1.0))
            m00, m11 = 1.0 / l00, 1.0 / l11
            m10 = -(l10 * m00) / l11
            info = np.stack([np.where(fin, a, 0.0) for a in (a00, a01, a11)], axis=1)
            cov = np.stack([np.where(ok, m00 * m00 + m10 * m10, inf), np.where(ok, m10 * m11, 0.0),
                            np.where(ok, m11 * m11, inf)], axis=1)
        else:
            a00, a01, a02, a11, a12, a22 = _seq_sum(np.stack(
                [ww * jx * jx, ww * jx * jy, ww * jx * jz, ww * jy * jy, ww * jy * jz, ww * jz * jz], axis=1))
            fin = (np.isfinite(a00) & np.isfinite(a01) & np.isfinite(a02) & np.isfinite(a11) & np.isfinite(a12)
                   & np.isfinite(a22))
            ok = fin & (a00 > SINGULAR * a00)
            l00 = np.sqrt(np.where(ok, a00, 1.0))
            l10, l20 = a01 / l00, a02 / l00
            t11 = a11 - l10 * l10
            ok = ok & (t11 > SINGULAR * a11) & np.isfinite(t11)
            l11 = np.sqrt(np.where(ok, t11, 1.0))
            l21 = (a12 - l20 * l10) / l11
            t22 = a22 - l20 * l20 - l21 * l21
            ok = ok & (t22 > SINGULAR * a22) & np.isfinite(t22)
            l22 = np.sqrt(np.where(ok, t22, 1.0))
            m00, m11, m22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
            m10 = -(l10 * m00) / l11
            m21 = -(l21 * m11) / l22
            m20 = -(l20 * m00 + l21 * m10) / l22
            info = np.stack([np.where(fin, a, 0.0) for a in (a00, a01, a02, a11, a12, a22)], axis=1)
            cov = np.stack([np.where(ok, m00 * m00 + m10 * m10 + m20 * m20, inf), np.where(ok, m10 * m11 + m20 * m21, 0.0),
                            np.where(ok, m20 * m22, 0.0), np.where(ok, m11 * m11 + m21 * m21, inf),
                            np.where(ok, m21 * m22, 0.0), np.where(ok, m22 * m22, inf)], axis=1)
    return info, cov, np.ascontiguousarray(r.T)


def solve_fix_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, plane=None, max_iter=60):
    """rmx_solve_batch_fix: (pos, cost, iters, info, cov, resid), the walk of k_solve (plane None) or k_solve_plane, then
    k_solve_fix at its pos"""
    if plane is None:
        pos, cost, it = kr.solve_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, max_iter)
    else:
        pos, cost, it = plane_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, plane, max_iter)
    return (pos, cost, it) + fix_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, pos, plane)


# -- the same quantities with numpy.linalg ----------------------------------------------------------------------------------
def sym(packed):
    """[W][3] (11 12 22) or [W][6] (xx xy xz yy yz zz) -> [W][n][n]"""
    packed = np.asarray(packed)
    n = {3: 2, 6: 3}[packed.shape[-1]]
    idx = np.zeros((n, n), int)
    k = 0
    for i in range(n):
        for j in range(i, n):
            idx[i, j] = idx[j, i] = k
            k += 1
    return packed[..., idx]


def fix_linalg(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, pos, plane=None):
    """J^T W J with @, its inverse with np.linalg.inv, the residuals with np.linalg.norm: (info [W][n][n], cov [W][n][n],
    resid [W][P], cond [W]); meant for positions where the information is regular"""
    buoys = np.asarray(buoy_xyz, np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs).reshape(-1, 2)
    pos = np.asarray(pos, np.float64)
    W = len(pos)
    d = (np.asarray(lag_int, np.float64) + np.asarray(lag_frac, np.float32).astype(np.float64)) * metres_per_sample
    wgt = np.ones(d.shape) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    v = pos[:, None, :] - buoys[None, :, :]                   # [W][B][3]
    n = np.linalg.norm(v, axis=2)
    unit = v / n[:, :, None]
    J = unit[:, pairs[:, 1], :] - unit[:, pairs[:, 0], :]     # [W][P][3]
    resid = n[:, pairs[:, 1]] - n[:, pairs[:, 0]] - d
    if plane is not None:
        E = np.asarray(plane, np.float64).reshape(3, 3)[1:]   # [2][3]
        J = J @ E.T
    info = np.transpose(J, (0, 2, 1)) @ (wgt[:, :, None] * J)
    return info, np.linalg.inv(info), resid, np.linalg.cond(info)


# -- scenes (the issue's appendix): lat, lng, alt on GeodeticCalculator's sphere ------------------------------------------------
FS_SCENE = 2.048e6
_FIVE = [(37.00, -122.00, 0.0), (37.08, -122.02, 0.0), (37.05, -121.90, 0.0), (36.95, -121.93, 0.0), (36.97, -122.08, 0.0)]
SCENES = {
    "sea5": (_FIVE, (37.02, -121.97, 0.0)),
    "sea4": (_FIVE[:4], (37.02, -121.97, 0.0)),
    "sea3": (_FIVE[:3], (37.04, -121.97, 0.0)),
    "heights6": ([(37.00, -122.00, 0.0), (37.08, -122.02, 900.0), (37.05, -121.90, 2500.0), (36.95, -121.93, 300.0),
                  (36.97, -122.08, 4000.0), (37.03, -121.99, 6000.0)], (37.02, -121.97, 1500.0)),
}


def scene(name):
    """(buoys [B][3] ECEF, emitter [3] ECEF, plane [9]): the tangent plane at the centroid's lat/lng, at the emitter's
    altitude"""
    from radio_mapper_amd.tdoa_processor import GeodeticCalculator as G
    stations, emitter = SCENES[name]
    buoys = np.array([G.lat_lng_to_xyz(*s) for s in stations])
    lat, lng, _ = G.xyz_to_lat_lng(*buoys.mean(axis=0))
    return buoys, np.array(G.lat_lng_to_xyz(*emitter)), as_plane(*G.tangent_plane(lat, lng, emitter[2]))


def noisy_lags(buoys, emitter, T, seed, fs=FS_SCENE):
    """all pairs; independent Gaussian lag noise with one sigma per pair drawn from 0.02 ... 0.2 samples; weight =
    1 / sigma_d^2 in float32.  Returns (pairs, lag_int [T][P], lag_frac, weight [T][P])"""
    rng = np.random.default_rng(seed)
    pairs = kr.all_pairs(len(buoys))
    mps = kr.metres_per_sample(fs)
    dist = np.linalg.norm(emitter[None, :] - buoys, axis=1)
    true = (dist[pairs[:, 1]] - dist[pairs[:, 0]]) / mps
    sigma = rng.uniform(0.02, 0.2, len(pairs))
    lag = true[None, :] + rng.normal(0.0, 1.0, (T, len(pairs))) * sigma[None, :]
    li = np.round(lag).astype(np.int32)
    wgt = np.tile((1.0 / (sigma * mps) ** 2).astype(np.float32), (T, 1))
    return pairs, li, (lag - li).astype(np.float32), wgt


def monte_carlo(name, plane_mode, T=2000, seed=1, max_iter=60):
    """T noisy windows of a scene through the kernel-order restatement.  Returns a dict: iters (mean), maxed (share of
    windows on max_iter), bias [n] (mean error, metres; plane coordinates or ECEF), var_ratio [n] (sample variance of the
    error over the mean predicted variance, marginal), nees (mean e^T info e), cost (mean), n, P, T and the raw arrays"""
    buoys, emitter, plane = scene(name)
    pairs, li, lf, wgt = noisy_lags(buoys, emitter, T, seed)
    mps = kr.metres_per_sample(FS_SCENE)
    pos, cost, it, info, cov, resid = solve_fix_kernel_order(buoys, pairs, li, lf, wgt, mps, plane if plane_mode else None,
                                                             max_iter)
    err = pos - emitter[None, :]
    if plane_mode:
        err = err @ plane.reshape(3, 3)[1:].T
    n = err.shape[1]
    info_m, cov_m = sym(info), sym(cov)
    nees = np.einsum("wi,wij,wj->w", err, info_m, err)
    return dict(iters=it.mean(), maxed=(it >= max_iter).mean(), bias=err.mean(axis=0),
                var_ratio=err.var(axis=0, ddof=1) / np.diagonal(cov_m, axis1=1, axis2=2).mean(axis=0), nees=nees.mean(),
                cost=cost.mean(), n=n, P=len(pairs), T=T, err=err, cov=cov_m, info=info_m, pos=pos, plane=plane,
                buoys=buoys, emitter=emitter)

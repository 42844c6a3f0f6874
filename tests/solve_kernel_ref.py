"""Kernel-order restatement of k_solve (radio-mapper_amd/csrc/solve_path.hpp), TEST INFRASTRUCTURE ONLY.

oracle/solve_ref.py states the Levenberg-Marquardt rule of rmx_solve_batch with numpy's own sums (`@`, np.linalg.solve,
mean), so it agrees with the kernel only where the walk is well conditioned.  This file follows the kernel operation by
operation instead: float64, the kernel's order of sums and products, one rounding per operation (the kernel is compiled
with fp contract(off); f64 divide and square root are correctly rounded on the device).  Each pair's terms are computed
elementwise over pairs and windows (the roundings of one pair and one window at a time), and every sum over the pairs is
a Python loop in list order (_seq_sum).  Its outputs are therefore the kernel's bit for bit, for every window, converged
or not.  Only + - * / and np.sqrt on float64 arrays are used: no np.sum, @, hypot or linalg, whose summation order is
numpy's business.

Per-window control flow runs through an index set of the windows still iterating: a finished window is never touched
again.  The NaN path is part of the contract (a centroid on a buoy gives 0/0 in every Jacobian entry, `d00 > 0` and
`fn < f` then compare false and the step is rejected), so everything runs under np.errstate(all="ignore")."""
import numpy as np

SPEED_OF_LIGHT = 299792458.0


def metres_per_sample(sample_rate_hz):
    """the kernel argument: computed once on the host as 299792458.0 / sample_rate_hz"""
    return SPEED_OF_LIGHT / float(sample_rate_hz)


def _seq_sum(terms):
    """sum over the leading axis in index order, one rounding per addition (np.sum adds pairwise)"""
    acc = np.zeros(terms.shape[1:])
    for t in terms:
        acc = acc + t
    return acc


def _norm_to(x, y, z, b):
    """sqrt((x-bx)*(x-bx) + (y-by)*(y-by) + (z-bz)*(z-bz)), summed left to right; x, y, z [n], b [P][3] -> [P][n]"""
    bx, by, bz = b[:, 0, None], b[:, 1, None], b[:, 2, None]
    return np.sqrt((x - bx) * (x - bx) + (y - by) * (y - by) + (z - bz) * (z - bz))


def _f_at(x, y, z, b1, b2, d, wgt):
    """the kernel's f_at lambda; b1, b2 [P][3] the buoys of every pair, d [P][n] metres, wgt [P][n] float64 or 1.0.  Every
    pair's term is computed elementwise (the same roundings as one pair at a time), then added in list order."""
    n1 = _norm_to(x, y, z, b1)
    n2 = _norm_to(x, y, z, b2)
    r = n2 - n1 - d
    return _seq_sum(wgt * r * r)


def solve_kernel_order(buoy_xyz, pairs, lag_int, lag_frac, weight, metres_per_sample, max_iter=60):
    """buoy_xyz [B][3] float64; pairs [P][2] int, used as given (repeats, reversed pairs and (i, i) included);
    lag_int int32 [W][P]; lag_frac float32 [W][P]; weight float32 [W][P] or None; metres_per_sample float (see
    metres_per_sample()).  Returns (pos float64 [W][3], cost float64 [W], iters int32 [W])."""
    buoys = np.ascontiguousarray(buoy_xyz, dtype=np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    li = np.asarray(lag_int, dtype=np.int32)
    lf = np.asarray(lag_frac, dtype=np.float32)
    W, P = li.shape
    assert lf.shape == (W, P) and len(pairs) == P and max_iter >= 1
    wg_all = None if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
    assert wg_all is None or wg_all.shape == (W, P)
    mps = np.float64(metres_per_sample)
    n_buoys = len(buoys)
    b1, b2 = buoys[pairs[:, 0]], buoys[pairs[:, 1]]      # [P][3]
    with np.errstate(all="ignore"):
        d_all = np.ascontiguousarray(((li.astype(np.float64) + lf.astype(np.float64)) * mps).T)      # [P][W]
        wg_all = 1.0 if wg_all is None else np.ascontiguousarray(wg_all.T)
        cx = cy = cz = np.float64(0.0)
        for b in range(n_buoys):
            cx = cx + buoys[b, 0]
            cy = cy + buoys[b, 1]
            cz = cz + buoys[b, 2]
        cx, cy, cz = cx / np.float64(n_buoys), cy / np.float64(n_buoys), cz / np.float64(n_buoys)
        px, py, pz = np.full(W, cx), np.full(W, cy), np.full(W, cz)
        lam = np.full(W, 1e-3)
        f = _f_at(px, py, pz, b1, b2, d_all, wg_all)
        it = np.zeros(W, np.int32)
        act = np.arange(W)                       # the windows still inside `while (it < max_iter)`
        while act.size:
            it[act] += 1
            x, y, z, lm, fa = px[act], py[act], pz[act], lam[act], f[act]
            d = d_all[:, act]
            ww = wg_all if np.ndim(wg_all) == 0 else wg_all[:, act]
            # every pair's terms elementwise, [P][n] ...
            v1x, v1y, v1z = x - b1[:, 0, None], y - b1[:, 1, None], z - b1[:, 2, None]
            v2x, v2y, v2z = x - b2[:, 0, None], y - b2[:, 1, None], z - b2[:, 2, None]
            n1 = np.sqrt(v1x * v1x + v1y * v1y + v1z * v1z)
            n2 = np.sqrt(v2x * v2x + v2y * v2y + v2z * v2z)
            r = n2 - n1 - d
            jx, jy, jz = v2x / n2 - v1x / n1, v2y / n2 - v1y / n1, v2z / n2 - v1z / n1
            # ... and the nine accumulators over the pairs in list order
            a00, a01, a02, a11, a12, a22, g0, g1, g2 = _seq_sum(np.stack(
                [ww * jx * jx, ww * jx * jy, ww * jx * jz, ww * jy * jy, ww * jy * jz, ww * jz * jz,
                 ww * jx * r, ww * jy * r, ww * jz * r], axis=1))
            d00, d11, d22 = a00 * (1.0 + lm), a11 * (1.0 + lm), a22 * (1.0 + lm)
            ok = d00 > 0.0
            l00 = np.sqrt(np.where(ok, d00, 1.0))
            l10, l20 = a01 / l00, a02 / l00
            t11 = d11 - l10 * l10
            ok = ok & (t11 > 0.0)
            l11 = np.sqrt(np.where(ok, t11, 1.0))
            l21 = (a12 - l20 * l10) / l11
            t22 = d22 - l20 * l20 - l21 * l21
            ok = ok & (t22 > 0.0)
            l22 = np.sqrt(np.where(ok, t22, 1.0))
            # (the kernel computes the step only `if (ok)`; here it is computed for all and used under the mask)
            y0 = -g0 / l00
            y1 = (-g1 - l10 * y0) / l11
            y2 = (-g2 - l20 * y0 - l21 * y1) / l22
            dz = y2 / l22
            dy = (y1 - l21 * dz) / l11
            dx = (y0 - l10 * dy - l20 * dz) / l00
            fn = _f_at(x + dx, y + dy, z + dz, b1, b2, d, ww)
            acc = ok & (fn < fa)                 # NaN compares false: a rejected step
            dn = np.sqrt(dx * dx + dy * dy + dz * dz)
            px[act] = np.where(acc, x + dx, x)
            py[act] = np.where(acc, y + dy, y)
            pz[act] = np.where(acc, z + dz, z)
            f[act] = np.where(acc, fn, fa)
            third = lm / 3.0
            lm_new = np.where(acc, np.where(third > 1e-12, third, 1e-12), lm * 4.0)
            lam[act] = lm_new
            stop = np.where(acc, dn < 1e-4, lm_new > 1e12) | (it[act] >= max_iter)
            act = act[~stop]
    return np.stack([px, py, pz], axis=1), f, it


# -- inputs shared by tests/test_solve_rule_cpu.py and tests/test_gpu_solve_exact.py ---------------------------------------
DEGENERATE_C = np.array([4000000.0, 100000.0, 4900000.0])
DEGENERATE_V = np.array([1000.0, 2000.0, 500.0])


def all_pairs(n_buoys):
    return np.array([(i, j) for i in range(n_buoys) for j in range(i + 1, n_buoys)], np.int32).reshape(-1, 2)


def seeded_lags(n_windows, n_pairs, seed, span=60):
    """lags that belong to no position: integers uniform in +-span samples, fractions uniform in +-0.5"""
    rng = np.random.default_rng(seed)
    li = rng.integers(-span, span + 1, (n_windows, n_pairs)).astype(np.int32)
    lf = rng.uniform(-0.5, 0.5, (n_windows, n_pairs)).astype(np.float32)
    return li, lf


def line_of_buoys(ks):
    """buoys c + k v: three of them at k = 1, 0, -1 put the centroid exactly on the middle buoy; the five at
    k = -3, -1, 0.5, 2, 4 are collinear with the centroid c + 0.5 v exactly on the third (tests/test_solve_rule_cpu.py
    pins that the sequential float64 sums land there)"""
    return np.array([DEGENERATE_C + k * DEGENERATE_V for k in ks])

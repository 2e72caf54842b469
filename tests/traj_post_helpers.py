"""References for trajectory post-processing (include/trk.h: trk_traj_spline_resample, trk_traj_waypoint_variance), in numpy.

spline64     the fp64 restatement: the slopes from a dense solve of the tridiagonal system (not the Thomas recurrence the kernel
             runs), the samples by the header's Hermite form.  Against the reference's own scipy route (tests/golden/traj_post.npz)
             it agrees to 1e-12 of the column's magnitude.
spline32     the kernel's arithmetic, operation by operation, in sequential fp32 -- what the tolerances below were measured with.
variance64   compute_variance_waypoints per problem in fp64, from the coordinate differences.

Tolerances of the GPU tests.
  position   |delta| <= C_P 2^-24 mag, mag = max_i |y_i| of the column.  spline32 against spline64 over 2000 random cases (N up to
             256, S up to 1024; test_traj_post_cpu.py re-measures it) reached at worst 4.59 x 2^-24 mag; C_P = 18.4 is 4 x that.
             The factor 4 covers a different rounding of the divisions and of any contraction, not a different algorithm.
  velocity   vel_mode 2: |delta| <= C_V 2^-24 mag (N - 1), same procedure; worst 8.71, C_V = 35.
  variance   relative 4 (dim + 4) 2^-24 per problem, a priori: a distance carries at most (dim + 4) / 2 roundings and its square twice
             that; the sums are fp64; by Cauchy-Schwarz S1^2 / n < S2 / 2, so the subtraction loses at most a factor 4.
The kernel's own worst ratios on the MI355X are recorded in DESIGN.md 6f."""
import numpy as np

C_P = 18.4
C_V = 35.0
EPS = 2.0 ** -24
VEL_MODES = {"zero": 0, "average": 1, "spline": 2}
N_PIVOTS = 32


def var_rtol(dim):
    return 4.0 * (dim + 4) * EPS


def sample_table(N, S):
    """segment and local parameter of every sample, from integers: (i [S], r [S]); tau = r / (S - 1); the last is (N - 2, S - 1)"""
    a = np.arange(S, dtype=np.int64) * (N - 1)
    i, r = a // (S - 1), a % (S - 1)
    i[-1], r[-1] = N - 2, S - 1
    return i, r


def slopes64(y):
    """y [..., N, D] fp64 -> the slopes ds/du at the knots, s_0 = s_{N-1} = 0, by a dense solve"""
    N = y.shape[-2]
    s = np.zeros_like(y)
    if N > 2:
        A = 4.0 * np.eye(N - 2) + np.eye(N - 2, k=1) + np.eye(N - 2, k=-1)
        b = 3.0 * (N - 1) * (y[..., 2:, :] - y[..., :-2, :])
        s[..., 1:-1, :] = np.linalg.solve(A, b)
    return s


def spline64(y, S, vel_mode="average", dt=0.02):
    """-> pos, vel [..., S, D] in fp64 (y is taken as it is, S dt as the kernel rounds it)"""
    y = np.asarray(y, np.float64)
    N = y.shape[-2]
    s = slopes64(y)
    i, r = sample_table(N, S)
    tau = (r / (S - 1.0))[:, None]
    y0, y1, s0, s1 = y[..., i, :], y[..., i + 1, :], s[..., i, :], s[..., i + 1, :]
    h = 1.0 / (N - 1)
    pos = y0 + (3 * tau ** 2 - 2 * tau ** 3) * (y1 - y0) + h * tau * (1 - tau) * ((1 - tau) * s0 - tau * s1)
    vel = np.zeros_like(pos)
    if VEL_MODES[vel_mode] == 1:
        vel[..., 1:-1, :] = (y[..., 1:2, :] - y[..., 0:1, :]) / np.float64(np.float32(np.float64(S) * np.float64(np.float32(dt))))
    elif VEL_MODES[vel_mode] == 2:
        vel = (N - 1) * 6 * tau * (1 - tau) * (y1 - y0) + (1 - tau) * (1 - 3 * tau) * s0 + tau * (3 * tau - 2) * s1
        vel[..., 0, :] = 0.0
        vel[..., -1, :] = 0.0
    return pos, vel


def pivots32():
    m, out = 0.25, []
    for _ in range(N_PIVOTS):
        out.append(np.float32(m))
        m = 1.0 / (4.0 - m)
    return out


def spline32(y, S, vel_mode="average", dt=0.02):
    """the kernel's arithmetic in sequential fp32, without contraction: y [..., N, D] fp32 -> pos, vel [..., S, D] fp32"""
    f = np.float32
    y = np.asarray(y, f)
    N = y.shape[-2]
    piv = pivots32()
    c3, c6, h = f(3.0 * (N - 1)), f(6.0 * (N - 1)), f(1.0 / (N - 1))
    s = np.zeros_like(y)
    with np.errstate(all="ignore"):
        g = np.zeros_like(y[..., 0, :])
        for i in range(1, N - 1):
            b = c3 * (y[..., i + 1, :] - y[..., i - 1, :])
            g = (b - g) * piv[min(i - 1, N_PIVOTS - 1)]
            s[..., i, :] = g
        sn = np.zeros_like(g)
        for i in range(N - 2, 0, -1):
            sn = s[..., i, :] - piv[min(i - 1, N_PIVOTS - 1)] * sn
            s[..., i, :] = sn
        i, r = sample_table(N, S)
        tau = (r.astype(f) / f(S - 1))[:, None]
        y0, y1, s0, s1 = y[..., i, :], y[..., i + 1, :], s[..., i, :], s[..., i + 1, :]
        om, dy = f(1) - tau, y1 - y0
        pos = (y0 + ((tau * tau) * (f(3) - f(2) * tau)) * dy) + ((h * tau) * om) * (om * s0 - tau * s1)
        pos = np.where(tau == 0, y0, pos)
        pos[..., -1, :] = y1[..., -1, :]
        vel = np.zeros_like(pos)
        if VEL_MODES[vel_mode] == 1:
            sdt = f(np.float64(S) * np.float64(f(dt)))
            vel[..., 1:-1, :] = (y[..., 1:2, :] - y[..., 0:1, :]) / sdt
        elif VEL_MODES[vel_mode] == 2:
            vel = (((c6 * tau) * om) * dy + (om * (f(1) - f(3) * tau)) * s0) + (tau * (f(3) * tau - f(2))) * s1
            vel[..., 0, :] = 0
            vel[..., -1, :] = 0
    return pos.astype(f), vel.astype(f)


def column_mag(y):
    """max_i |y_i| of every column, shaped to broadcast against the samples: [..., 1, D]"""
    return np.abs(np.asarray(y, np.float64)).max(-2, keepdims=True)


def variance64(x, c0, dim):
    """x [P, K, H, Sd] -> [P] fp64: sum_t var(triu(cdist(x_t, x_t), 1).view(-1)), unbiased over all K^2 entries"""
    x = np.asarray(x, np.float64)[..., c0:c0 + dim]
    P, K, H, _ = x.shape
    n = float(K * K)
    out = np.zeros(P)
    iu = np.triu_indices(K, 1)
    with np.errstate(all="ignore"):
        for p in range(P):
            for t in range(H):
                pts = x[p, :, t]
                d = np.sqrt(((pts[iu[0]] - pts[iu[1]]) ** 2).sum(-1))
                s1, s2 = d.sum(), (d * d).sum()
                out[p] += (s2 - s1 * s1 / n) / (n - 1.0) if K > 1 else np.nan
    return out


def variance_cdist32(x, c0, dim):
    """the same value the way torch.cdist forms distances above 25 rows -- |a|^2 + |b|^2 - 2 a.b in fp32 -- with fp64 sums: what the
    kernel must NOT compute (the clustered case tells the two apart)"""
    f = np.float32
    x = np.asarray(x, f)[..., c0:c0 + dim]
    P, K, H, _ = x.shape
    n = float(K * K)
    out = np.zeros(P)
    iu = np.triu_indices(K, 1)
    for p in range(P):
        for t in range(H):
            pts = x[p, :, t]
            sq = (pts * pts).sum(-1, dtype=f)
            d2 = (sq[:, None] + sq[None, :]) - f(2) * (pts @ pts.T).astype(f)
            d = np.sqrt(np.maximum(d2, f(0)))[iu].astype(np.float64)
            s1, s2 = d.sum(), (d * d).sum()
            out[p] += (s2 - s1 * s1 / n) / (n - 1.0)
    return out

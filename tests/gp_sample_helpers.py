"""References for trk_gp_prior_sample and trk_traj_select_best (include/trk.h, "GP-prior sampling and best-particle pick").

sample64: the header's formulas in fp64, with `mag` -- the same formulas with every term replaced by its absolute value -- per output
element.  Every comparison of the kernel with sample64 allows  tol(H) * mag,  tol(H) = (2 H + 16) 2^-24:  the a-priori bound for any
association of at most 2 H additions over leaves that carry a few roundings each.
sample32: the same formulas as a sequential walk in fp32, one rounding per operation (what the bound must cover with room).
dense_conditioning: the conditional Gaussian of the prior's block-tridiagonal precision, for checking sample64 itself.
select_best_ref: trk_traj_select_best in numpy."""
import numpy as np

F32 = np.float32


def tol(H):
    return (2 * H + 16) * 2.0 ** -24


def constants(dt, sigma, H, rounded=True):
    """l00, l10, l11 (the Cholesky factor of Q = sigma^2 [[dt^3/3, dt^2/2], [dt^2/2, dt]]) and theta = (H - 1) dt from the fp32 dt and
    sigma, formed in double; rounded: once to fp32, as the library passes them to its kernel"""
    dt, sigma = float(F32(dt)), float(F32(sigma))
    c = (sigma * dt ** 1.5 / np.sqrt(3.0), sigma * (np.sqrt(3.0) / 2.0) * np.sqrt(dt), sigma * np.sqrt(dt) / 2.0, (H - 1) * dt)
    return tuple(float(F32(v)) for v in c) if rounded else c


def hermite(s):
    """the four weights of (r_p, r_v) in q and in qd, up to theta: (3 s^2 - 2 s^3, s^3 - s^2, 6 s - 6 s^2, 3 s^2 - 2 s)"""
    return 3 * s ** 2 - 2 * s ** 3, s ** 3 - s ** 2, 6 * s - 6 * s ** 2, 3 * s ** 2 - 2 * s


def sample64(start, goal, eps, dt, sigma, n_particles, pin_vel=False, start_vel=None, goal_vel=None, q_min=None, q_max=None,
             rounded=True):
    """start, goal (P, D); eps (P K, H - 1, D, 2) -> q, qd, mag_q, mag_qd, each (P K, H, D) fp64"""
    eps = np.asarray(eps, np.float64)
    N, T, D, _ = eps.shape
    H, K = T + 1, int(n_particles)
    rep = lambda a: np.repeat(np.asarray(a, np.float64), K, axis=0)
    st, go = rep(start), rep(goal)
    assert st.shape == (N, D)
    l00, l10, l11, theta = constants(dt, sigma, H, rounded)
    dt = float(F32(dt))
    p, v, mp, mv = (np.zeros((N, H, D)) for _ in range(4))
    p[:, 0], mp[:, 0] = st, np.abs(st)
    if pin_vel:
        sv, gv = rep(start_vel), rep(goal_vel)
        v[:, 0], mv[:, 0] = sv, np.abs(sv)
    for t in range(T):
        e0, e1 = eps[:, t, :, 0], eps[:, t, :, 1]
        p[:, t + 1] = p[:, t] + dt * v[:, t] + l00 * e0
        v[:, t + 1] = v[:, t] + (l10 * e0 + l11 * e1)
        mp[:, t + 1] = mp[:, t] + dt * mv[:, t] + np.abs(l00 * e0)
        mv[:, t + 1] = mv[:, t] + np.abs(l10 * e0) + np.abs(l11 * e1)
    tt = np.arange(H, dtype=np.float64).reshape(1, H, 1)
    rp, mrp = (go - p[:, T])[:, None], (np.abs(go) + mp[:, T])[:, None]
    if pin_vel:
        rv, mrv = (gv - v[:, T])[:, None], (np.abs(gv) + mv[:, T])[:, None]
        hpp, hpv, hvp, hvv = hermite(tt / T)
        q = p + hpp * rp + theta * hpv * rv
        qd = v + (hvp / theta) * rp + hvv * rv
        mq = mp + np.abs(hpp) * mrp + theta * np.abs(hpv) * mrv
        mqd = mv + (np.abs(hvp) / theta) * mrp + np.abs(hvv) * mrv
        qd[:, 0], qd[:, T] = sv, gv
    else:
        q = p + tt * dt * (rp / theta)
        qd = v + rp / theta
        mq = mp + tt * dt * (mrp / theta)
        mqd = mv + mrp / theta
    if q_min is not None:
        q[:, 1:T] = np.clip(q[:, 1:T], np.asarray(q_min, np.float64), np.asarray(q_max, np.float64))
    q[:, 0], q[:, T] = st, go
    return q, qd, mq, mqd


def sample32(start, goal, eps, dt, sigma, n_particles, pin_vel=False, start_vel=None, goal_vel=None):
    """the same formulas, a sequential walk with every operation rounded to fp32 (no limits) -> q, qd (P K, H, D) fp32"""
    eps = np.asarray(eps, F32)
    N, T, D, _ = eps.shape
    H, K = T + 1, int(n_particles)
    rep = lambda a: np.repeat(np.asarray(a, F32), K, axis=0)
    st, go = rep(start), rep(goal)
    l00, l10, l11, theta = (F32(c) for c in constants(dt, sigma, H))
    dt = F32(dt)
    p, v = np.zeros((N, H, D), F32), np.zeros((N, H, D), F32)
    p[:, 0] = st
    if pin_vel:
        sv, gv = rep(start_vel), rep(goal_vel)
        v[:, 0] = sv
    for t in range(T):
        e0, e1 = eps[:, t, :, 0], eps[:, t, :, 1]
        p[:, t + 1] = (p[:, t] + dt * v[:, t]) + l00 * e0
        v[:, t + 1] = v[:, t] + (l10 * e0 + l11 * e1)
    tt = np.arange(H, dtype=F32).reshape(1, H, 1)
    rp = (go - p[:, T])[:, None]
    if pin_vel:
        rv = (gv - v[:, T])[:, None]
        s = tt / F32(T)
        one, two, three, six = F32(1), F32(2), F32(3), F32(6)
        q = (p + (three * s * s - two * s * s * s) * rp) + (theta * (s * s * s - s * s)) * rv
        qd = (v + ((six * s - six * s * s) / theta) * rp) + (three * s * s - two * s) * rv
        qd[:, 0], qd[:, T] = sv, gv
    else:
        vs = rp / theta
        q = p + (tt * dt) * vs
        qd = v + vs
    q[:, 0], q[:, T] = st, go
    assert q.dtype == F32 and qd.dtype == F32
    return q, qd


def dense_conditioning(H, dt, sigma, pin_vel, start, goal, start_vel=0.0, goal_vel=0.0):
    """One coordinate.  The prior's density over x = (p_0, v_0, ..., p_T, v_T) is exp(-sum_t 1/2 e_t^T Q^-1 e_t), e_t = Phi x_t - x_{t+1},
    Q^-1 = [[a, b], [b, c]] with the a, b, c of trk_gp_prior_cost_grad.  Conditioned on the pinned components (positions of both ends;
    with pin_vel their velocities too) -> (indices of the free components, their mean, their covariance), by dense linear algebra."""
    s2 = 1.0 / (sigma * sigma)
    a, b, c = 12.0 * s2 / dt ** 3, -6.0 * s2 / dt ** 2, 4.0 * s2 / dt
    Qi = np.array([[a, b], [b, c]])
    Phi = np.array([[1.0, dt], [0.0, 1.0]])
    n = 2 * H
    L = np.zeros((n, n))
    for t in range(H - 1):
        G = np.zeros((2, n))
        G[:, 2 * t:2 * t + 2] = Phi
        G[:, 2 * t + 2:2 * t + 4] = -np.eye(2)
        L += G.T @ Qi @ G
    pinned = {0: start, n - 2: goal}
    if pin_vel:
        pinned.update({1: start_vel, n - 1: goal_vel})
    Cidx = sorted(pinned)
    Fidx = [i for i in range(n) if i not in pinned]
    xc = np.array([pinned[i] for i in Cidx])
    cov = np.linalg.inv(L[np.ix_(Fidx, Fidx)])
    mean = -cov @ L[np.ix_(Fidx, Cidx)] @ xc
    return Fidx, mean, cov


def select_best_ref(score, is_free, n_particles):
    """-> best (P,) int64 (row p K + k, -1 without a candidate), best_score (P,) fp32 (+inf without), n_free (P,) int32"""
    K = int(n_particles)
    s = np.asarray(score, F32).reshape(-1, K)
    P = s.shape[0]
    fr = np.ones((P, K), bool) if is_free is None else (np.asarray(is_free).reshape(P, K) != 0)
    best, bs = np.full(P, -1, np.int64), np.full(P, np.inf, F32)
    for p in range(P):
        for k in range(K):
            if fr[p, k] and not np.isnan(s[p, k]) and (best[p] < 0 or s[p, k] < bs[p]):
                best[p], bs[p] = p * K + k, s[p, k]
    return best, bs, fr.sum(1).astype(np.int32)

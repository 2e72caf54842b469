"""References for the sampling-based trajectory update (include/trk.h: trk_traj_softmin_weights, trk_traj_weighted_update), in numpy:
weights64, the fp64 restatement of both weight modes; update32, the update restated operation by operation in fp32 with the
header's association (chunks of 64 particles in ascending k, then the chunks in ascending order); update64, its fp64 form, and
update_bound, the a-priori bound between any fp32 association and the fp64 form."""
import numpy as np

EPS = 2.0 ** -24
W_RTOL, W_ATOL = 2.0 ** -23, 2.0 ** -126      # one rounding to fp32, a factor 2 for the fp64 terms; below 2^-126 a weight is not judged
CHUNK = 64
F32 = np.float32


def weights64(cost, K, temperature, mode="trajectory", valid=None):
    """cost (P K, H) or (P K,) -> (w, ess) in float64: w (P K,) and ess (P,) in the trajectory mode, w (P K, H) and ess (P, H) per
    way point.  temperature is rounded to fp32 first, as the entry receives it."""
    c = np.asarray(cost, np.float32).astype(np.float64)
    if c.ndim == 1:
        c = c[:, None]
    N, H = c.shape
    P = N // K
    lam = float(np.float32(temperature))
    ok = np.ones(N, bool) if valid is None else np.asarray(valid).reshape(N) != 0
    with np.errstate(all="ignore"):
        v = (c.sum(1, keepdims=True) if mode == "trajectory" else c).reshape(P, K, -1)      # (P, K, 1 or H)
        cand = ok.reshape(P, K, 1) & np.isfinite(v)
        any_ = cand.any(1, keepdims=True)
        lo = np.where(cand, v, np.inf).min(1, keepdims=True)
        hi = np.where(cand, v, -np.inf).max(1, keepdims=True)
        if mode == "trajectory":
            arg = -(v - lo) / lam
        else:
            arg = np.where(hi > lo, -(v - lo) / ((hi - lo) * lam), 0.0)
        a = np.where(cand, np.exp(np.where(cand, arg, 0.0)), 0.0)
        Z = a.sum(1, keepdims=True)
        w = np.where(cand, a / np.where(any_, Z, 1.0), 0.0)
        ess = np.where(any_, Z * Z / np.where(any_, (a * a).sum(1, keepdims=True), 1.0), 0.0)
    if mode == "trajectory":
        return w.reshape(N), ess.reshape(P)
    return w.reshape(N, H), ess.reshape(P, H)


def _shapes(mean, x, w):
    mean = np.asarray(mean)
    P, H, D = mean.shape
    K = x.shape[0] // P
    wb = np.asarray(w).reshape(P, K, H, 1) if np.asarray(w).ndim == 2 else np.asarray(w).reshape(P, K, 1, 1)
    return P, K, H, D, np.asarray(x).reshape(P, K, H, D), wb


def _finish(mean, r, pin, lo, hi):
    if lo is not None:
        with np.errstate(invalid="ignore"):
            r = np.where(r < lo, lo, r)
            r = np.where(r > hi, hi, r)
    r = r.astype(mean.dtype)
    if pin & 1:
        r[:, 0] = mean[:, 0]
    if pin & 2:
        r[:, -1] = mean[:, -1]
    return r


def update32(mean, x, w, step, pin=0, lo=None, hi=None):
    """the kernel's arithmetic in fp32, every operation rounded once: d = x - mean, acc = acc + w * d (skipped by select where w is
    exactly 0), chunk sums from +0 in ascending k, chunk 0's sum + chunk 1's + ..., out = mean + step * acc (mean's bits at step = 0)"""
    mean = np.asarray(mean, F32)
    P, K, H, D, x4, wb = _shapes(mean, np.asarray(x, F32), np.asarray(w, F32))
    total = None
    with np.errstate(all="ignore"):
        for c0 in range(0, K, CHUNK):
            acc = np.zeros((P, H, D), F32)
            for k in range(c0, min(K, c0 + CHUNK)):
                wk = np.broadcast_to(wb[:, k], (P, H, D))
                d = x4[:, k] - mean
                s = acc + wk * d
                acc = np.where(wk != 0, s, acc)
            total = acc if total is None else total + acc
        r = mean + F32(step) * total
    if F32(step) == 0:
        r = mean.copy()
    return _finish(mean, r, pin, None if lo is None else np.asarray(lo, F32), None if hi is None else np.asarray(hi, F32))


def update64(mean, x, w, step, pin=0, lo=None, hi=None):
    """-> (out, mag) in float64: the same expression in fp64 (a particle of weight 0 does not enter, whatever its row holds) and
    mag = |mean| + |step| sum_k |w_k| |x_k - mean|"""
    mean = np.asarray(mean, np.float32).astype(np.float64)
    P, K, H, D, x4, wb = _shapes(mean, np.asarray(x, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64))
    st = float(np.float32(step))
    with np.errstate(all="ignore"):
        term = np.where(wb != 0, wb * np.where(wb != 0, x4 - mean[:, None], 0.0), 0.0)
    r = mean + st * term.sum(1)
    mag = np.abs(mean) + abs(st) * np.abs(term).sum(1)
    as64 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)
    return _finish(mean, r, pin, as64(lo), as64(hi)), mag


def update_bound(K, mag):
    """|any fp32 association - fp64| <= (K + 3) 2^-24 mag: per term the difference, the product and its addition to a sum of at most K
    terms, then the product with step and the final addition, each one rounding of a quantity bounded by mag"""
    return (K + 3) * EPS * mag

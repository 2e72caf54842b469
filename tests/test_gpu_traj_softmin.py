"""The sampling-based trajectory update on the GPU (csrc/trk_traj_softmin.hip).  trk_traj_softmin_weights against the fp64
restatement weights64 of traj_softmin_helpers (validated on the CPU: test_traj_softmin_cpu.py) within 2^-23 w + 2^-126 per weight and
2^-23 relative on ess; its zeros, its underflow, the independence of a problem's bits from the batch.  trk_traj_weighted_update
against the fp32 restatement update32 bit for bit and against update64 within (K + 3) 2^-24 (|mean| + |step| sum |w| |x - mean|);
pins, limits, aliasing, skipped particles, the buffers' edges, one captured replay.  PlanningTask.sampling_optimizer on the Panda
and the 3-D point mass against the same iteration written in torch and numpy; the example."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import traj_softmin_helpers as sm
import helpers as hp
from torch_robotics_amd import _abi, _lib, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
KS = (1, 2, 3, 63, 64, 65, 130, 257)
MODES = ("trajectory", "waypoint")
TINY = 2.0 ** -126


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return (host(t) if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)).view(np.uint32)


def check_weights(c, K, lam, mode, valid=None, no_underflow=True):
    """-> (w, ess, reference w, worst ratio): every weight within 2^-23 w + 2^-126 of weights64 and exactly 0 where the reference
    has no candidate; ess within 2^-23 relative"""
    w, ess = ops.traj_softmin_weights(dev(c), K, lam, mode, None if valid is None else dev(valid))
    rw, re = sm.weights64(c, K, lam, mode, valid)
    assert w.shape == rw.shape and ess.shape == re.shape and w.dtype == ess.dtype == torch.float32
    if no_underflow:                                       # the case is built so that every candidate's weight is judged
        assert rw[rw > 0].size == 0 or rw[rw > 0].min() >= TINY
    ew = np.abs(host(w).astype(np.float64) - rw)
    assert (ew <= sm.W_RTOL * rw + sm.W_ATOL).all(), (K, lam, mode)
    assert (host(w)[rw == 0] == 0).all()
    ee = np.abs(host(ess).astype(np.float64) - re)
    assert (ee <= sm.W_RTOL * re).all(), (K, lam, mode)
    worst = float((ew[rw > 0] / (sm.W_RTOL * rw[rw > 0])).max()) if (rw > 0).any() else 0.0
    return w, ess, rw, worst


def random_cost(rng, P, K, H, lam):
    """scores whose soft-min keeps every weight above 2^-126: the summed scores of a problem spread over at most min(4, 60 lambda),
    so the exponent stays below 60 + ln K < 87"""
    return (rng.random((P * K, H)) * (min(4.0, 60.0 * lam) / H)).astype(np.float32)


# weights 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_weights_against_the_fp64_restatement(K):
    rng = np.random.default_rng(100 + K)
    worst = 0.0
    for H in (1, 3, 64, 65):
        for P in (1, 5):
            for lam in (0.1, 1.0, 50.0):
                c = random_cost(rng, P, K, H, lam)
                for mode in MODES:
                    w, ess, rw, r = check_weights(c, K, lam, mode)
                    worst = max(worst, r)
                    sums = host(w).astype(np.float64).reshape(P, K, -1).sum(1)
                    assert np.allclose(sums, 1.0, rtol=0, atol=K * 2.0 ** -23)
    # a vector of summed scores is horizon 1
    c = random_cost(rng, 5, K, 1, 1.0)
    w1, e1 = ops.traj_softmin_weights(dev(c[:, 0]), K, 1.0)
    w2, e2 = ops.traj_softmin_weights(dev(c), K, 1.0)
    assert torch.equal(w1, w2) and torch.equal(e1, e2)
    print(f"  K={K}: worst |w - w64| / (2^-23 w) = {worst:.3f}")


# weights 2 --------------------------------------------------------------------------------------------------------------------
def test_weights_underflow_leaves_the_minimum_alone():
    """lambda = 1e-3: every exponent but the minimum's is below -500; the minimum's weight is 1, the rest lie in [0, 2^-126]"""
    rng = np.random.default_rng(7)
    for K, H in ((3, 1), (65, 3), (257, 64)):
        P = 4
        c = (0.5 + rng.random((P * K, H))).astype(np.float32)
        best = rng.integers(0, K, P)
        c.reshape(P, K, H)[np.arange(P), best] = 0.0
        for mode in MODES:
            w, ess = ops.traj_softmin_weights(dev(c), K, 1e-3, mode)
            wh = host(w).astype(np.float64).reshape(P, K, -1)
            top = wh[np.arange(P), best]
            assert (np.abs(top - 1.0) <= sm.W_RTOL + sm.W_ATOL).all()
            rest = wh.copy()
            rest[np.arange(P), best] = 0.0
            assert (rest >= 0).all() and (rest <= TINY).all()
            assert (np.abs(host(ess).astype(np.float64) - 1.0) <= sm.W_RTOL).all()


# weights 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 3, 64, 65, 257))
def test_weights_equal_scores_non_finite_scores_and_rejected_particles(K):
    rng = np.random.default_rng(200 + K)
    P, H = 6, 5
    # all scores equal: 1 / K and ess = K in both modes
    c = np.full((P * K, H), 1.25, np.float32)
    for mode in MODES:
        w, ess, rw, _ = check_weights(c, K, 1.0, mode)
        assert (np.abs(host(w) - 1.0 / K) <= sm.W_RTOL / K).all() and (np.abs(host(ess) - K) <= sm.W_RTOL * K).all()
    # hi == lo at one way point only
    c = random_cost(rng, P, K, H, 1.0)
    c[:, 2] = 0.75
    w, ess, rw, _ = check_weights(c, K, 0.1, "waypoint")
    assert (np.abs(host(w)[:, 2] - 1.0 / K) <= sm.W_RTOL / K).all()
    # NaN, +inf and -inf scores, and valid zeroing particles and whole problems (problems 1 and 4 have no candidate)
    c = random_cost(rng, P, K, H, 1.0)
    flat = c.reshape(-1)
    flat[rng.integers(0, flat.size, 1 + flat.size // 7)] = np.nan
    flat[rng.integers(0, flat.size, 1 + flat.size // 9)] = np.inf
    flat[rng.integers(0, flat.size, 1 + flat.size // 9)] = -np.inf
    valid = (rng.random(P * K) < 0.7).astype(np.uint8) * rng.integers(1, 256, P * K).astype(np.uint8)
    valid.reshape(P, K)[[1, 4]] = 0
    for mode in MODES:
        for v in (None, valid, valid != 0):
            w, ess, rw, _ = check_weights(c, K, 1.0, mode, None if v is None else v.astype(np.uint8))
            assert torch.isfinite(w).all() and torch.isfinite(ess).all()
            if v is not None:
                assert (bits(w).reshape(P, K, -1)[[1, 4]] == 0).all() and (bits(ess).reshape(P, -1)[[1, 4]] == 0).all()
        wb, eb = ops.traj_softmin_weights(dev(c), K, 1.0, mode, dev(valid != 0))          # bool flags are the same bytes
        wu, eu = ops.traj_softmin_weights(dev(c), K, 1.0, mode, dev(valid))
        assert torch.equal(wb, wu) and torch.equal(eb, eu)


# weights 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H", [(3, 65), (64, 1), (65, 3), (257, 64)])
def test_a_problems_weights_do_not_depend_on_the_batch(K, H):
    rng = np.random.default_rng(300 + K)
    P = 7
    c = random_cost(rng, P, K, H, 1.0)
    valid = (rng.random(P * K) < 0.8).astype(np.uint8)
    other = random_cost(rng, 4, K, H, 1.0)
    for mode in MODES:
        run = lambda cc, vv: ops.traj_softmin_weights(dev(cc), K, 0.5, mode, dev(vv))
        w, ess = run(c, valid)
        w2, ess2 = run(c, valid)
        assert torch.equal(w, w2) and torch.equal(ess, ess2)                       # two calls
        for p in range(P):                                                         # alone
            w1, e1 = run(c[p * K:(p + 1) * K], valid[p * K:(p + 1) * K])
            assert torch.equal(w1, w[p * K:(p + 1) * K]) and torch.equal(e1, ess[p:p + 1]), p
        for a, b in ((0, 3), (3, 7)):                                              # the batch in two calls
            w1, e1 = run(c[a * K:b * K], valid[a * K:b * K])
            assert torch.equal(w1, w[a * K:b * K]) and torch.equal(e1, ess[a:b])
        w1, e1 = run(np.concatenate([other, c]), np.concatenate([np.ones(4 * K, np.uint8), valid]))      # behind others
        assert torch.equal(w1[4 * K:], w) and torch.equal(e1[4:], ess)


# update 1 ---------------------------------------------------------------------------------------------------------------------
def draw_update(rng, P, K, H, D, per_wp):
    mean = rng.standard_normal((P, H, D)).astype(np.float32)
    x = (mean[:, None] + 0.3 * rng.standard_normal((P, K, H, D))).astype(np.float32).reshape(P * K, H, D)
    mode = "waypoint" if per_wp else "trajectory"
    w = sm.weights64((rng.random((P * K, H)) * 3).astype(np.float32), K, 0.5, mode)[0].astype(np.float32)
    return mean, x, w


def check_update(mean, x, w, step, pin=0, lo=None, hi=None, got=None):
    """bit for bit update32, and within the a-priori bound of update64 -> (the result, the worst fraction of the bound)"""
    P = mean.shape[0]
    K = x.shape[0] // P
    if got is None:
        got = ops.traj_weighted_update(dev(mean), dev(x), dev(w), step, pin, None if lo is None else dev(lo), None if hi is None else dev(hi))
    assert got.shape == mean.shape and got.dtype == torch.float32
    want = sm.update32(mean, x, w, step, pin, lo, hi)
    assert np.array_equal(bits(got), want.view(np.uint32)), (K, mean.shape, step, pin)
    ref, mag = sm.update64(mean, x, w, step, pin, lo, hi)
    e = np.abs(host(got).astype(np.float64) - ref)
    bound = sm.update_bound(K, mag)
    assert (e <= bound).all()
    return got, float((e[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("K", KS)
def test_update_against_the_fp32_restatement_bit_for_bit(K):
    rng = np.random.default_rng(400 + K)
    worst = 0.0
    for H in (1, 3, 64):
        for D in (1, 3, 7, 14, 32):
            for per_wp in (False, True):
                mean, x, w = draw_update(rng, 2, K, H, D, per_wp)
                for step in (0.0, 0.5, 1.0):
                    got, r = check_update(mean, x, w, step)
                    worst = max(worst, r)
                    if step == 0.0:
                        assert np.array_equal(bits(got), mean.view(np.uint32))
    print(f"  K={K}: worst |kernel - fp64| / ((K + 3) 2^-24 mag) = {worst:.3f}")


# update 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,D", [(3, 1, 7), (3, 2, 1), (64, 3, 14), (65, 64, 7), (257, 3, 32)])
def test_update_pins_limits_and_aliasing(K, H, D):
    rng = np.random.default_rng(500 + K + H)
    P = 3
    lo, hi = np.full(D, -0.6, np.float32) + 0.1 * rng.random(D).astype(np.float32), np.full(D, 0.7, np.float32)
    for per_wp in (False, True):
        mean, x, w = draw_update(rng, P, K, H, D, per_wp)
        mean[0, 0, 0], mean[1, -1, -1] = -0.0, -0.0                   # a pinned -0 keeps its sign
        for pin in (0, 1, 2, 3):
            free, _ = check_update(mean, x, w, 0.5, pin)
            if pin & 1:
                assert np.array_equal(bits(free[:, 0]), mean[:, 0].view(np.uint32))
            if pin & 2:
                assert np.array_equal(bits(free[:, -1]), mean[:, -1].view(np.uint32))
            lim, _ = check_update(mean, x, w, 0.5, pin, lo, hi)
            fh, lh = host(free), host(lim)
            unpinned = np.ones((P, H, D), bool)
            if pin & 1:
                unpinned[:, 0] = False
            if pin & 2:
                unpinned[:, -1] = False
            assert (lh[unpinned] >= np.broadcast_to(lo, lh.shape)[unpinned]).all() and (lh[unpinned] <= np.broadcast_to(hi, lh.shape)[unpinned]).all()
            kept = (fh >= lo) & (fh <= hi) | ~unpinned                # untouched by the clamp: the bits of the run without limits
            assert np.array_equal(lh[kept].view(np.uint32), fh[kept].view(np.uint32))
            assert np.array_equal(lh[~kept], np.where(fh < lo, lo, hi)[~kept])
        # out aliasing mean
        m = dev(mean)
        back = ops.traj_weighted_update(m, dev(x), dev(w), 1.0, 3, dev(lo), dev(hi), out=m)
        assert back is m
        check_update(mean, x, w, 1.0, 3, lo, hi, got=m)


# update 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 64, 130))
def test_update_skips_rejected_and_underflowed_particles(K):
    """a rejected particle's row is NaN / inf: its weight is exactly 0 and the output stays finite; a weight that underflowed to 0 is
    skipped the same way; a NaN in a particle that has weight stays in its own element"""
    rng = np.random.default_rng(600 + K)
    P, H, D = 3, 5, 7
    mean = rng.standard_normal((P, H, D)).astype(np.float32)
    x = (mean[:, None] + 0.3 * rng.standard_normal((P, K, H, D))).astype(np.float32).reshape(P * K, H, D)
    c = (rng.random((P * K, H)) * 2).astype(np.float32)
    valid = np.ones(P * K, np.uint8)
    rejected = [0, K - 1, K + K // 2, 2 * K]
    valid[rejected] = 0
    for j, fill in zip(rejected, (np.nan, np.inf, -np.inf, np.nan)):
        x[j] = fill
    for mode in MODES:
        w = ops.traj_softmin_weights(dev(c), K, 0.5, mode, dev(valid))[0]
        assert (bits(w)[rejected] == 0).all()
        got, _ = check_update(mean, x, host(w), 1.0, 3)
        assert torch.isfinite(got).all()
    # underflow: the weights of lambda = 1e-3 are exactly 0 for every particle but the best, whose rows are the only finite ones
    c = (0.5 + rng.random((P * K, 1))).astype(np.float32)
    best = rng.integers(0, K, P)
    c.reshape(P, K)[np.arange(P), best] = 0.0
    w = ops.traj_softmin_weights(dev(c), K, 1e-3)[0]
    assert (bits(w).reshape(P, K)[np.arange(P), best] == np.float32(1).view(np.uint32)).all() and int((bits(w) != 0).sum()) == P
    xb = np.full_like(x, np.nan)
    xb.reshape(P, K, H, D)[np.arange(P), best] = (mean + 0.3 * rng.standard_normal((P, H, D))).astype(np.float32)
    got, _ = check_update(mean, xb, host(w), 1.0, 0)
    assert torch.isfinite(got).all()
    # step 1 and weight 1: mean + (x - mean)
    assert np.array_equal(bits(got), (mean + (xb.reshape(P, K, H, D)[np.arange(P), best] - mean)).view(np.uint32))
    # a NaN under a non-zero weight reaches its own element only
    xn = x.copy()
    xn[rejected] = 0.0
    xn[1, 2, 3] = np.nan
    wn = np.full(P * K, 1.0 / K, np.float32)
    got = ops.traj_weighted_update(dev(mean), dev(xn), dev(wn), 1.0, 0)
    bad = ~torch.isfinite(got)
    assert int(bad.sum()) == 1 and bool(bad[0, 2, 3])


# update 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,D,per_wp", [(3, 64, 7, False), (64, 3, 32, True), (65, 3, 7, True), (257, 64, 3, False)])
def test_a_problems_update_does_not_depend_on_the_batch(K, H, D, per_wp):
    rng = np.random.default_rng(700 + K)
    P = 5
    mean, x, w = draw_update(rng, P, K, H, D, per_wp)
    lo, hi = np.full(D, -0.8, np.float32), np.full(D, 0.9, np.float32)
    run = lambda m, xx, ww: ops.traj_weighted_update(dev(m), dev(xx), dev(ww), 0.5, 3, dev(lo), dev(hi))
    out = run(mean, x, w)
    assert torch.equal(run(mean, x, w), out)                                                        # two calls
    for p in range(P):                                                                              # alone
        assert torch.equal(run(mean[p:p + 1], x[p * K:(p + 1) * K], w[p * K:(p + 1) * K])[0], out[p]), p
    for a, b in ((0, 2), (2, 5)):                                                                   # the batch in two calls
        assert torch.equal(run(mean[a:b], x[a * K:b * K], w[a * K:b * K]), out[a:b])
    om, ox, ow = draw_update(rng, 3, K, H, D, per_wp)                                               # behind others
    assert torch.equal(run(np.concatenate([om, mean]), np.concatenate([ox, x]), np.concatenate([ow, w]))[3:], out)


# edges ------------------------------------------------------------------------------------------------------------------------
def off_by_one_float(a, pad=64, fill=-777.25, dtype=torch.float32):
    """a copy of `a` inside a larger buffer filled with a sentinel, starting 4 bytes past a 16-byte boundary -> (view, whole buffer)"""
    n = int(np.prod(a.shape))
    whole = torch.full((pad + 1 + n + pad,), fill, device=DEV, dtype=dtype)
    assert whole.data_ptr() % 16 == 0
    view = whole[pad + 1:pad + 1 + n].view(a.shape)
    view.copy_(dev(a))
    assert view.data_ptr() % 16 == 4
    return view, whole


def edges_intact(whole, n, pad=64, fill=-777.25):
    edge = torch.cat([whole[:pad + 1], whole[pad + 1 + n:]])
    return edge.numel() == 2 * pad + 1 and bool((edge == fill).all())


@pytest.mark.parametrize("K,H,D", [(3, 3, 7), (64, 65, 3), (130, 64, 7), (257, 1, 1), (257, 3, 2)])
@pytest.mark.parametrize("mode", (0, 1))
def test_sentinels_around_the_outputs_at_four_byte_alignment(K, H, D, mode):
    """cost, w, ess, x, mean, the limits, out and the workspace all 4 bytes off a 16-byte boundary: the words either side of w, ess and
    out keep their value and the results are those of the aligned calls, bit for bit"""
    rng = np.random.default_rng(800 + K)
    P = 3
    c = random_cost(rng, P, K, H, 1.0)
    mean, x, _ = draw_update(rng, P, K, H, D, False)
    lo, hi = np.full(D, -0.8, np.float32), np.full(D, 0.9, np.float32)
    ref_w, ref_ess = ops.traj_softmin_weights(dev(c), K, 1.0, MODES[mode])
    ref_out = ops.traj_weighted_update(dev(mean), dev(x), ref_w, 0.5, 3, dev(lo), dev(hi))
    cv, xv, mv, lov, hiv = (off_by_one_float(a)[0] for a in (c, x, mean, lo, hi))
    (w, w_all), (ess, ess_all), (out, out_all) = (off_by_one_float(np.zeros(s, np.float32)) for s in (tuple(ref_w.shape), tuple(ref_ess.shape), mean.shape))
    nbytes = _lib.lib().trk_traj_weighted_update_workspace_bytes(P, K, H, D)
    work, _ = off_by_one_float(np.zeros(max(nbytes // 4, 1), np.float32))
    wbytes = _lib.lib().trk_traj_softmin_weights_workspace_bytes(P, K, H, mode)
    wwork = torch.empty((wbytes // 8 + 1,), device=DEV, dtype=torch.float64)         # doubles: 8-byte aligned
    s = _abi.Softmin(1.0, mode, K)
    u = _abi.WeightedUpdate(0.5, 3, K, mode)
    with torch.cuda.device(DEV):
        rc = _lib.lib().trk_traj_softmin_weights(C.byref(s), cv.data_ptr(), None, P, H, w.data_ptr(), ess.data_ptr(), wwork.data_ptr(), wbytes,
                                                 ops._stream_of(DEV))
        assert rc == 0, _lib.lib().trk_last_error().decode()
        rc = _lib.lib().trk_traj_weighted_update(C.byref(u), xv.data_ptr(), mv.data_ptr(), w.data_ptr(), lov.data_ptr(), hiv.data_ptr(), P, H, D,
                                                 out.data_ptr(), work.data_ptr(), nbytes, ops._stream_of(DEV))
        assert rc == 0, _lib.lib().trk_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(w, ref_w) and torch.equal(ess, ref_ess) and torch.equal(out, ref_out)
    assert edges_intact(w_all, ref_w.numel()) and edges_intact(ess_all, ref_ess.numel()) and edges_intact(out_all, mean.size)


def test_one_replay_of_a_captured_weights_and_update_pair_equals_the_eager_result():
    rng = np.random.default_rng(9)
    P, K, H, D = 4, 300, 24, 7                         # both entries take their two-launch form
    c, valid = dev(random_cost(rng, P, K, H, 1.0)), dev((rng.random(P * K) < 0.8).astype(np.uint8))
    mean, x, _ = (dev(a) for a in draw_update(rng, P, K, H, D, False))
    lo, hi = dev(np.full(D, -0.8, np.float32)), dev(np.full(D, 0.9, np.float32))

    def work():
        res = []
        for mode in MODES:
            w, ess = ops.traj_softmin_weights(c, K, 0.5, mode, valid)
            res += [w, ess, ops.traj_weighted_update(mean, x, w, 0.5, 3, lo, hi)]
        return res

    eager = work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = work()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


def test_the_python_wrappers_name_the_shapes_they_refuse():
    c = torch.zeros((6, 4), **TA)
    with pytest.raises(ValueError, match="not a multiple of n_particles"):
        ops.traj_softmin_weights(c, 4, 1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.traj_softmin_weights(c.double(), 3, 1.0)
    with pytest.raises(ValueError, match=r"valid must be a contiguous bool / uint8 vector of shape \(6,\)"):
        ops.traj_softmin_weights(c, 3, 1.0, valid=torch.ones(5, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="temperature must be finite and > 0"):
        ops.traj_softmin_weights(c, 3, 0.0)
    with pytest.raises(NotImplementedError, match=r"TRK_SOFTMIN_MAX_PARTICLES \(4096\)"):
        ops.traj_softmin_weights(torch.zeros((4097, 1), **TA), 4097, 1.0)
    mean, x = torch.zeros((2, 4, 3), **TA), torch.zeros((6, 4, 3), **TA)
    with pytest.raises(ValueError, match=r"x must be a \(problems \* n_particles, 4, 3\)"):
        ops.traj_weighted_update(mean, torch.zeros((5, 4, 3), **TA), torch.zeros(5, **TA))
    with pytest.raises(ValueError, match=r"weights must be a contiguous float32 tensor of shape \(6,\)"):
        ops.traj_weighted_update(mean, x, torch.zeros(5, **TA))
    with pytest.raises(ValueError, match=r"weights must be a contiguous float32 tensor of shape \(6, 4\)"):
        ops.traj_weighted_update(mean, x, torch.zeros((6, 3), **TA))
    with pytest.raises(ValueError, match="q_min and q_max come together"):
        ops.traj_weighted_update(mean, x, torch.zeros(6, **TA), q_min=torch.zeros(3, **TA))
    with pytest.raises(ValueError, match=r"pin must be 0 \.\. 3"):
        ops.traj_weighted_update(mean, x, torch.zeros(6, **TA), pin=4)
    with pytest.raises(ValueError, match="step must be finite"):
        ops.traj_weighted_update(mean, x, torch.zeros(6, **TA), step=float("nan"))
    w, ess = ops.traj_softmin_weights(torch.zeros((0, 4), **TA), 3, 1.0, "waypoint")             # an empty batch
    assert w.shape == (0, 4) and ess.shape == (0, 4)


# the plan ---------------------------------------------------------------------------------------------------------------------
SIGMA_GP, SIGMA_NOISE = 1.0, 0.3


def make_task(robot):
    return tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=getattr(tra, robot)(tensor_args=TA), obstacle_cutoff_margin=0.03,
                            clamp_sdf=True, tensor_args=TA)


def straight_lines(task, P, H, T=5.0):
    D = task.robot.q_dim
    torch.manual_seed(3)
    start = task.random_coll_free_q(n_samples=P).reshape(P, D)
    goal = task.random_coll_free_q(n_samples=P).reshape(P, D)
    s = torch.linspace(0.0, 1.0, H, **TA).reshape(1, H, 1)
    q = (start[:, None] + s * (goal - start)[:, None]).contiguous()
    qd = ((goal - start) / T)[:, None].expand(P, H, D).contiguous()
    return q, qd


@pytest.mark.parametrize("robot,H", [("RobotPanda", 24), ("RobotPointMass3D", 100)])
@pytest.mark.parametrize("mode", MODES)
def test_one_iteration_of_the_plan_against_torch_and_numpy(robot, H, mode):
    """step(1) with a fixed eps against the same iteration written out: the noise from ops.gp_prior_sample with zero ends, added to
    the means, the interior clamped, the cost from the task and the prior, the weights from weights64 on that cost, and the update in
    fp64.  Within (K + 5) 2^-24 (|mean| + |step| sum |w| |x - mean|): the update's (K + 3) and 2 for the weights' own 2^-23."""
    task = make_task(robot)
    P, K, D = 3, 8, task.robot.q_dim
    dt, lam, step = 5.0 / H, 2.0, 0.7
    q, qd = straight_lines(task, P, H)
    q0, qd0 = q.clone(), qd.clone()
    plan = task.sampling_optimizer(q, qd, dt, SIGMA_GP, K, SIGMA_NOISE, lam, mode=mode, w_coll=5.0, gp_weight=0.01, step=step)
    eps = torch.randn((P * K, H - 1, D, 2), generator=torch.Generator(device=DEV).manual_seed(2), **TA)
    first = plan.step(1, eps=eps)
    # the same iteration, written out
    e0 = eps.clone()
    e0.view(P, K, H - 1, D, 2)[:, 0] = 0
    zero = torch.zeros((P, D), **TA)
    nq, nqd = ops.gp_prior_sample(zero, zero, H, dt, SIGMA_NOISE, K, eps=e0)
    assert (nq.view(P, K, H, D)[:, 0] == 0).all() and (nq[:, 0] == 0).all() and (nq[:, -1] == 0).all()
    lo, hi = task.robot.q_min.to(DEV).reshape(D), task.robot.q_max.to(DEV).reshape(D)
    xq = (q0[:, None] + nq.view(P, K, H, D)).reshape(P * K, H, D)
    xq[:, 1:-1] = torch.minimum(torch.maximum(xq[:, 1:-1], lo), hi)
    xqd = (qd0[:, None] + nqd.view(P, K, H, D)).reshape(P * K, H, D)
    with torch.no_grad():
        cost = 5.0 * task.compute_collision_cost(xq) + (0.01 / H) * ops.gp_prior_cost(xq, xqd, dt, SIGMA_GP)[:, None]
    assert cost.shape == (P * K, H)
    w = sm.weights64(host(cost), K, lam, mode)[0].astype(np.float32)
    for got, mean, x, pin, lim in ((q, q0, xq, 3, (host(lo), host(hi))), (qd, qd0, xqd, 0, (None, None))):
        ref, mag = sm.update64(host(mean), host(x), w, step, pin, *lim)
        e = np.abs(host(got).astype(np.float64) - ref)
        assert (e <= (K + 5) * sm.EPS * mag).all()
    assert torch.equal(q[:, 0], q0[:, 0]) and torch.equal(q[:, -1], q0[:, -1])
    assert not torch.equal(q, q0) and not torch.equal(qd, qd0)
    # the returned cost is particle 0's: the mean's own
    want = host(cost).astype(np.float64).reshape(P, K, H)[:, 0]
    assert (np.abs(host(first).astype(np.float64) - want.sum(1)) <= H * sm.EPS * np.abs(want).sum(1)).all()
    assert plan.ess.shape == ((P,) if mode == "trajectory" else (P, H)) and (plan.ess >= 1 - 1e-6).all() and (plan.ess <= K + 1e-3).all()


@pytest.mark.parametrize("robot,H", [("RobotPanda", 24), ("RobotPointMass3D", 100)])
def test_three_iterations_of_the_plan_keep_the_ends_the_limits_and_return_the_first_cost(robot, H):
    task = make_task(robot)
    P, K, D = 3, 8, task.robot.q_dim
    dt = 5.0 / H
    for mode, pin_vel in (("trajectory", False), ("waypoint", True)):
        q, qd = straight_lines(task, P, H)
        if pin_vel:
            qd[:, 0], qd[:, -1] = 0.0, 0.0
        q0, qd0 = q.clone(), qd.clone()
        gen = torch.Generator(device=DEV).manual_seed(4)
        plan = task.sampling_optimizer(q, qd, dt, SIGMA_GP, K, SIGMA_NOISE, 1.0 if mode == "trajectory" else 0.1, mode=mode, w_coll=5.0,
                                       gp_weight=0.01, pin_vel=pin_vel, generator=gen)
        want = plan.cost(q0, qd0).double()                              # the initial mean, evaluated separately
        first = plan.step(3)
        assert first.shape == (P,)
        assert (torch.abs(first.double() - want.sum(1)) <= H * sm.EPS * want.abs().sum(1)).all()
        assert torch.equal(q[:, 0], q0[:, 0]) and torch.equal(q[:, -1], q0[:, -1])
        if pin_vel:
            assert torch.equal(qd[:, 0], qd0[:, 0]) and torch.equal(qd[:, -1], qd0[:, -1])
        assert torch.isfinite(q).all() and torch.isfinite(qd).all()
        lo, hi = task.robot.q_min.to(DEV), task.robot.q_max.to(DEV)
        assert (q[:, 1:-1] >= lo).all() and (q[:, 1:-1] <= hi).all()
        assert not torch.equal(q, q0)


@pytest.mark.parametrize("robot", ["panda", "point3d"])
@pytest.mark.parametrize("mode", MODES)
def test_the_example_runs(robot, mode):
    spec = importlib.util.spec_from_file_location("plan_sampling", Path(hp.ROOT) / "examples" / "plan_sampling.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after = mod.main(robot=robot, problems=3, horizon=12, particles=4, iters=2, mode=mode, verbose=False)
    assert 0 <= before <= 3 and 0 <= after <= 3

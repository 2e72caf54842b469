"""Multi-particle planning on the GPU (csrc/trk_gp_sample.hip): trk_gp_prior_sample against the fp64 reference sample64 of
gp_sample_helpers (validated on the CPU: tests/test_gp_sample_cpu.py) within tol(H) * mag = (2 H + 16) 2^-24 * mag, its endpoint
bits, its clamp, the independence of a trajectory's bits from its place in the batch, the buffers' edges and the isolation of a
non-finite noise row to bit equality; trk_traj_select_best against a numpy restatement; one captured replay; the route through the
task on the Panda and the 3-D point mass; the example."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import gp_sample_helpers as gs
import helpers as hp
from torch_robotics_amd import _abi, _lib, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
PARAMS = ((5.0 / 64, 2.0), (5.0 / 128, 0.1))          # (dt, sigma)
# (H, D, P, K): every horizon of {2, 3, 31, 64, 65, 100, 256} with several D of {1, 3, 7, 32} and each (P, K) of {(1, 1), (3, 5),
# (7, 3)} -- part-filled workgroups, a problem's particles across workgroups -- and the D at which the launch takes another
# instantiation (4 | 5, 8 | 9, 16 | 17)
CASES = [(2, 1, 1, 1), (2, 32, 7, 3), (2, 7, 3, 5), (3, 3, 3, 5), (3, 7, 1, 1), (3, 32, 7, 3), (31, 7, 3, 5), (31, 1, 7, 3), (31, 32, 1, 1),
         (64, 7, 7, 3), (64, 3, 3, 5), (64, 32, 1, 1), (64, 1, 3, 5), (65, 3, 7, 3), (65, 7, 3, 5), (65, 32, 1, 1), (100, 7, 7, 3),
         (100, 32, 3, 5), (100, 1, 1, 1), (100, 3, 7, 3), (256, 3, 3, 5), (256, 32, 7, 3), (256, 1, 7, 3), (256, 7, 1, 1),
         (64, 4, 3, 5), (64, 5, 3, 5), (64, 8, 7, 3), (64, 9, 7, 3), (31, 16, 3, 5), (31, 17, 3, 5)]


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint32)


def draw(seed, H, D, P, K):
    """start, goal, start_vel, goal_vel (P, D) and eps (P K, H - 1, D, 2), unit normals in fp32; limits that clip some way points"""
    rng = np.random.default_rng(seed)
    st, go, sv, gv = (rng.standard_normal((P, D)).astype(np.float32) for _ in range(4))
    eps = rng.standard_normal((P * K, H - 1, D, 2)).astype(np.float32)
    lo = (-1.5 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    hi = (1.5 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    return st, go, sv, gv, eps, lo, hi


def run(st, go, sv, gv, eps, dt, sigma, K, pin, lim=None):
    H = eps.shape[1] + 1
    vel = (dev(sv), dev(gv)) if pin else (None, None)
    lims = (None, None) if lim is None else (dev(lim[0]), dev(lim[1]))
    return ops.gp_prior_sample(dev(st), dev(go), H, dt, sigma, K, vel[0], vel[1], eps=dev(eps), q_min=lims[0], q_max=lims[1])


def check_close(got, ref, mag, H, what):
    err = np.abs(host(got).astype(np.float64) - ref)
    worst = float((err[mag > 0] / (gs.tol(H) * mag[mag > 0])).max()) if (mag > 0).any() else 0.0
    print(f"  {what}: worst |kernel - fp64| / (tol(H) mag) = {worst:.3f}")
    assert (err <= gs.tol(H) * mag).all(), what
    return worst


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "H%d-D%d-P%d-K%d" % c)
def test_the_kernel_against_the_fp64_reference(case):
    """both pin modes, limits off and on, both (dt, sigma): values within tol(H) mag of sample64; the endpoints are the inputs' bits;
    with limits the interior lies inside them and every element the clamp left alone has the bits of the run without limits"""
    H, D, P, K = case
    st, go, sv, gv, eps, lo, hi = draw(1000 + H * 37 + D, H, D, P, K)
    rep = lambda a: np.repeat(a, K, 0)
    for dt, sigma in PARAMS:
        for pin in (False, True):
            ref = gs.sample64(st, go, eps, dt, sigma, K, pin, sv, gv)
            q, qd = run(st, go, sv, gv, eps, dt, sigma, K, pin)
            assert q.shape == qd.shape == (P * K, H, D)
            check_close(q, ref[0], ref[2], H, f"q dt={dt:.4f} sigma={sigma} pin_vel={pin}")
            check_close(qd, ref[1], ref[3], H, f"qd dt={dt:.4f} sigma={sigma} pin_vel={pin}")
            assert np.array_equal(bits(q[:, 0]), rep(st).view(np.uint32)) and np.array_equal(bits(q[:, -1]), rep(go).view(np.uint32))
            if pin:
                assert np.array_equal(bits(qd[:, 0]), rep(sv).view(np.uint32)) and np.array_equal(bits(qd[:, -1]), rep(gv).view(np.uint32))
            refl = gs.sample64(st, go, eps, dt, sigma, K, pin, sv, gv, q_min=lo, q_max=hi)
            ql, qdl = run(st, go, sv, gv, eps, dt, sigma, K, pin, lim=(lo, hi))
            check_close(ql, refl[0], refl[2], H, f"clamped q dt={dt:.4f} sigma={sigma} pin_vel={pin}")
            assert torch.equal(qdl, qd)                                             # the clamp does not touch qd
            assert np.array_equal(bits(ql[:, 0]), rep(st).view(np.uint32)) and np.array_equal(bits(ql[:, -1]), rep(go).view(np.uint32))
            inner, raw = host(ql)[:, 1:-1], host(q)[:, 1:-1]
            assert (inner >= lo).all() and (inner <= hi).all()
            kept = (raw >= lo) & (raw <= hi)
            assert np.array_equal(inner[kept].view(np.uint32), raw[kept].view(np.uint32))
            assert np.array_equal(inner[~kept], np.where(raw < lo, lo, hi)[~kept])


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", [(2, 7), (31, 7), (64, 7), (65, 3), (100, 32), (256, 3), (256, 32)])
@pytest.mark.parametrize("pin", (False, True))
def test_a_trajectorys_bits_depend_only_on_its_own_inputs(H, D, pin):
    """the whole batch (7 problems x 3 particles) against: each problem alone; the batch in two calls; one particle per problem (21
    problems with the starts and goals repeated, the same eps rows); and the batch behind four more problems"""
    P, K = 7, 3
    dt, sigma = PARAMS[0]
    st, go, sv, gv, eps, lo, hi = draw(77 + H + D, H, D, P, K)
    q, qd = run(st, go, sv, gv, eps, dt, sigma, K, pin, lim=(lo, hi))
    for p in range(P):
        q1, qd1 = run(st[p:p + 1], go[p:p + 1], sv[p:p + 1], gv[p:p + 1], eps[p * K:(p + 1) * K], dt, sigma, K, pin, lim=(lo, hi))
        assert torch.equal(q1, q[p * K:(p + 1) * K]) and torch.equal(qd1, qd[p * K:(p + 1) * K]), p
    for a, b in ((0, 3), (3, 7)):
        q2, qd2 = run(st[a:b], go[a:b], sv[a:b], gv[a:b], eps[a * K:b * K], dt, sigma, K, pin, lim=(lo, hi))
        assert torch.equal(q2, q[a * K:b * K]) and torch.equal(qd2, qd[a * K:b * K])
    rep = lambda x: np.repeat(x, K, 0)
    q3, qd3 = run(rep(st), rep(go), rep(sv), rep(gv), eps, dt, sigma, 1, pin, lim=(lo, hi))
    assert torch.equal(q3, q) and torch.equal(qd3, qd)
    o = draw(5, H, D, 4, K)
    cat = lambda x, y: np.concatenate([x, y], 0)
    q4, qd4 = run(cat(o[0], st), cat(o[1], go), cat(o[2], sv), cat(o[3], gv), cat(o[4], eps), dt, sigma, K, pin, lim=(lo, hi))
    assert torch.equal(q4[4 * K:], q) and torch.equal(qd4[4 * K:], qd)


# 3 ---------------------------------------------------------------------------------------------------------------------------
def raw_sample(st, go, sv, gv, eps, lo, hi, dt, sigma, P, K, H, D, pin, q, qd):
    """the C entry on caller-made device tensors (any alignment)"""
    s = _abi.GpSample(dt, sigma, K, int(pin))
    p = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(DEV):
        rc = _lib.lib().trk_gp_prior_sample(C.byref(s), p(st), p(go), p(sv), p(gv), p(eps), p(lo), p(hi), P, H, D, p(q), p(qd),
                                            ops._stream_of(DEV))
    assert rc == 0, _lib.lib().trk_last_error().decode()


def off_by_one_float(a, pad=64, fill=np.float32(-777.25)):
    """a copy of `a` inside a larger buffer filled with a sentinel, starting 4 bytes past an 8-byte boundary -> (view, whole buffer)"""
    n = int(np.prod(a.shape))
    whole = torch.full((pad + 1 + n + pad,), float(fill), **TA)
    assert whole.data_ptr() % 8 == 0
    view = whole[pad + 1:pad + 1 + n].view(a.shape)
    view.copy_(dev(a))
    assert view.data_ptr() % 8 == 4
    return view, whole


@pytest.mark.parametrize("H,D,P,K", [(3, 7, 3, 5), (64, 7, 7, 3), (100, 32, 3, 5), (256, 3, 3, 5)])
@pytest.mark.parametrize("pin", (False, True))
def test_sentinels_around_the_outputs_at_four_byte_alignment(H, D, P, K, pin):
    """q, qd, eps and the per-problem rows all 4 bytes off an 8-byte boundary: the words either side of q and qd keep their value,
    and the results are those of the aligned call, bit for bit"""
    dt, sigma = PARAMS[1]
    st, go, sv, gv, eps, lo, hi = draw(31 + H, H, D, P, K)
    ref_q, ref_qd = run(st, go, sv, gv, eps, dt, sigma, K, pin, lim=(lo, hi))
    ins = [off_by_one_float(a)[0] for a in (st, go, sv, gv, eps, lo, hi)]
    (q, q_all), (qd, qd_all) = (off_by_one_float(np.zeros((P * K, H, D), np.float32)) for _ in range(2))
    raw_sample(*ins[:2], *(ins[2:4] if pin else (None, None)), *ins[4:], dt, sigma, P, K, H, D, pin, q, qd)
    torch.cuda.synchronize()
    assert torch.equal(q, ref_q) and torch.equal(qd, ref_qd)
    n = P * K * H * D
    for whole in (q_all, qd_all):
        edge = torch.cat([whole[:65], whole[65 + n:]])
        assert edge.numel() == 129 and (edge == -777.25).all()


def test_a_nan_noise_row_stays_in_its_trajectory():
    for H, D, P, K in ((64, 7, 7, 3), (3, 3, 3, 5), (100, 32, 3, 5)):
        for pin in (False, True):
            dt, sigma = PARAMS[0]
            st, go, sv, gv, eps, lo, hi = draw(9 + H, H, D, P, K)
            q, qd = run(st, go, sv, gv, eps, dt, sigma, K, pin)
            bad = eps.copy()
            j = P * K // 2
            bad[j] = np.nan
            qn, qdn = run(st, go, sv, gv, bad, dt, sigma, K, pin)
            others = [i for i in range(P * K) if i != j]
            assert torch.equal(qn[others], q[others]) and torch.equal(qdn[others], qd[others])
            assert torch.isnan(qn[j, 1:-1]).all() and torch.equal(qn[j, 0], q[j, 0]) and torch.equal(qn[j, -1], q[j, -1])


# 4 ---------------------------------------------------------------------------------------------------------------------------
def scores_and_flags(seed, P, K):
    """scores on a coarse grid (exact ties are common) with NaN, +-inf and +-0 sprinkled in; flags with whole problems colliding"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, (P, K)).astype(np.float32) * np.float32(0.5)
    special = rng.integers(0, 12, (P, K))
    s[special == 0] = np.nan
    s[special == 1] = np.inf
    s[special == 2] = -np.inf
    s[special == 3] = -0.0
    fr = (rng.random((P, K)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (P, K)).astype(np.uint8)     # any non-zero byte is free
    fr[::5] = 0                       # all colliding
    s[3::7] = np.nan                  # no usable score at all
    return s.reshape(-1), fr.reshape(-1)


@pytest.mark.parametrize("K", [1, 3, 64, 65, 130])
def test_selection_against_numpy(K):
    P = 37
    s, fr = scores_and_flags(K, P, K)
    for flags in (fr, None):
        want = gs.select_best_ref(s, flags, K)
        best, bs, nf = ops.traj_select_best(dev(s), None if flags is None else dev(flags), K)
        assert best.dtype == torch.int64 and bs.dtype == torch.float32 and nf.dtype == torch.int32
        assert np.array_equal(host(best), want[0])
        assert np.array_equal(host(bs).view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(host(nf), want[2])
    want = gs.select_best_ref(s, fr, K)
    assert (want[0][::5] == -1).all() and np.isinf(want[1][::5]).all() and (want[1][::5] > 0).all() and (want[2][::5] == 0).all()
    # bool flags are the same bytes; the result does not depend on how problems are batched
    best_b = ops.traj_select_best(dev(s), dev(fr != 0), K)[0]
    assert np.array_equal(host(best_b), want[0])
    for a, b in ((0, 1), (1, 20), (20, 37)):
        part = ops.traj_select_best(dev(s[a * K:b * K]), dev(fr[a * K:b * K]), K)
        assert np.array_equal(host(part[0]), np.where(want[0][a:b] < 0, -1, want[0][a:b] - a * K))
        assert np.array_equal(host(part[2]), want[2][a:b])


def test_selection_ties_zeros_empty_batch_and_nullable_outputs():
    # the first of equal scores; -0.0 ties 0.0; a NaN is never the winner, an infinity may be
    s = np.array([1.0, 1.0, 0.5, 0.5, 0.0, -0.0, -0.0, 0.0, np.nan, np.inf, np.inf, np.nan, np.nan, -np.inf, 2.0, -np.inf], np.float32)
    best, bs, nf = ops.traj_select_best(dev(s), None, 4)
    assert host(best).tolist() == [2, 4, 9, 13] and host(nf).tolist() == [4, 4, 4, 4]
    assert np.array_equal(host(bs).view(np.uint32), s[[2, 4, 9, 13]].view(np.uint32))
    # an empty batch
    best, bs, nf = ops.traj_select_best(torch.empty((0,), **TA), None, 4)
    assert best.shape == bs.shape == nf.shape == (0,)
    # best_score and n_free are optional
    sd, out = dev(s), torch.full((4,), -5, device=DEV, dtype=torch.int64)
    with torch.cuda.device(DEV):
        rc = _lib.lib().trk_traj_select_best(sd.data_ptr(), None, 4, 4, out.data_ptr(), None, None, ops._stream_of(DEV))
    assert rc == 0 and host(out).tolist() == [2, 4, 9, 13]


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_one_replay_of_a_captured_sample_and_pick_equals_the_eager_result():
    H, D, P, K = 64, 7, 5, 4
    dt, sigma = PARAMS[0]
    st, go, sv, gv, eps, lo, hi = (dev(a) for a in draw(4, H, D, P, K))

    def work():
        q, qd = ops.gp_prior_sample(st, go, H, dt, sigma, K, sv, gv, eps=eps, q_min=lo, q_max=hi)
        return (q, qd) + ops.traj_select_best(ops.traj_diff_norm_sum(q, 0, D), None, K)

    eager = work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = work()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
    assert (eager[2] >= 0).all()


# 6 ---------------------------------------------------------------------------------------------------------------------------
SIGMA_TASK = 0.3


@pytest.mark.parametrize("robot", ["RobotPanda", "RobotPointMass3D"])
def test_through_the_task(robot):
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=getattr(tra, robot)(tensor_args=TA), obstacle_cutoff_margin=0.03,
                            clamp_sdf=True, tensor_args=TA)
    D, P, K, H = task.robot.q_dim, 6, 4, 16
    torch.manual_seed(11)
    start = task.random_coll_free_q(n_samples=P).reshape(P, D)
    goal = task.random_coll_free_q(n_samples=P).reshape(P, D)
    goal[1] = start[1]                 # a problem whose particles hover around one collision-free configuration
    gen = torch.Generator(device=DEV).manual_seed(5)
    q, qd = task.sample_gp_trajs(start, goal, K, H, 5.0 / H, SIGMA_TASK, generator=gen)
    assert q.shape == qd.shape == (P * K, H, D) and q.dtype == torch.float32 and q.device == DEV
    rep = lambda x: x.repeat_interleave(K, 0)
    assert torch.equal(q[:, 0], rep(start)) and torch.equal(q[:, -1], rep(goal))
    lo, hi = task.robot.q_min.to(DEV), task.robot.q_max.to(DEV)
    assert (q[:, 1:-1] >= lo).all() and (q[:, 1:-1] <= hi).all()
    # the same generator state gives the same draw, eps passed in gives that draw, pin_vel pins zero velocities
    eps = torch.randn((P * K, H - 1, D, 2), generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    q2, qd2 = task.sample_gp_trajs(start, goal, K, H, 5.0 / H, SIGMA_TASK, eps=eps)
    assert torch.equal(q2, q) and torch.equal(qd2, qd)
    free_q, _ = task.sample_gp_trajs(start, goal, K, H, 5.0 / H, SIGMA_TASK, eps=eps, clamp_to_limits=False)
    assert torch.equal(torch.minimum(torch.maximum(free_q, lo), hi)[:, 1:-1], q[:, 1:-1])
    _, qd3 = task.sample_gp_trajs(start, goal, K, H, 5.0 / H, SIGMA_TASK, eps=eps, pin_vel=True)
    assert (qd3[:, 0] == 0).all() and (qd3[:, -1] == 0).all()
    # the pick against get_trajs_collision_and_free + a masked argmin in torch; problem 0 leaves the joint limits with every particle
    trajs = torch.cat([q, qd], -1).contiguous()
    trajs[0:K, 1:-1, :D] = 1e3
    best_trajs, best, solved = task.select_best_trajs(trajs, K)
    _, _, _, free_idxs, _ = task.get_trajs_collision_and_free(trajs, return_indices=True)
    free = torch.zeros(P * K, dtype=torch.bool, device=DEV)
    free[free_idxs.reshape(-1).long()] = True
    score = ops.traj_diff_norm_sum(trajs, 0, D)
    want_solved = free.view(P, K).any(1)
    masked = torch.where(free, score, torch.full_like(score, float("inf"))).view(P, K)
    want = torch.where(want_solved, masked.argmin(1), score.view(P, K).argmin(1)) + torch.arange(P, device=DEV) * K
    print(f"{robot}: {int(free.sum())} of {P * K} particles free, {int(want_solved.sum())} of {P} problems solved")
    assert torch.equal(solved, want_solved) and not bool(solved[0]) and bool(solved.any())
    assert torch.equal(best, want) and torch.equal(best_trajs, trajs[want])
    # a score of the caller's: the negated length picks the longest free particle
    _, best_long, solved_long = task.select_best_trajs(trajs, K, score=-score)
    masked = torch.where(free, -score, torch.full_like(score, float("inf"))).view(P, K)
    want_long = torch.where(want_solved, masked.argmin(1), (-score).view(P, K).argmin(1)) + torch.arange(P, device=DEV) * K
    assert torch.equal(best_long, want_long) and torch.equal(solved_long, want_solved)


@pytest.mark.parametrize("model", ["links", "point3d"])
def test_the_example_runs(model):
    spec = importlib.util.spec_from_file_location("plan_particles", Path(hp.ROOT) / "examples" / "plan_particles.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    line, particles = mod.main(problems=4, particles=3, horizon=8, iters=1, model=model, verbose=False)
    assert 0 <= line <= 4 and 0 <= particles <= 4

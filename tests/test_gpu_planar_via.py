"""The 2-D point mass's via-point term (csrc/trk_planar.hip: via_segment, k_planar_traj_via) behind trk_scene2d_traj_via_cost_grad and
trk_scene2d_traj_via_adam_steps, on the synthetic scenes of tests/golden/pointmass2d_synth_*.npz.

Off means off (w_via = 0 and H = 1 give the existing calls' bits); the via cost is pinned bit for bit to the existing kernels on the
materialised via points (which carries over what tests/test_gpu_planar2d_edges.py establishes per point, kinks included) and checked
independently against helpers.planar64; the fold of the gradient onto the way points is held to its rounding bound and shown to see a
swapped fold; the three terms together, the Adam update, the grouping of iterations, the pins, the isolation of trajectories from a
non-finite neighbour, and the route through the task, a captured graph and the example.  Cases and bounds: planar_traj_helpers."""
import ctypes as C

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import planar_traj_helpers as pt
import test_gpu_planar2d_edges as edges
import test_gpu_planar_traj as tp
from helpers import rel_err
from torch_robotics_amd import _abi, _lib, ops

pytestmark = pytest.mark.gpu

DEV, TA, LR = tp.DEV, tp.TA, tp.LR
dev, host, inputs, params_of = tp.dev, tp.host, tp.inputs, tp.params_of
CASES = tp.CASES
# the one-segment trajectory, 85 trajectories per workgroup, the WAVE form and both sides of it, trajectories over 2 - 4 wavefronts, a
# ragged last workgroup, the limit
SHAPES = [(1, 2), (3, 3), (5, 63), (4, 64), (3, 65), (2, 128), (7, 200), (2, 256), (37, 64)]
N_INTERP = (1, 2, 5)
EPS = 2.0 ** -24
_refs = {}


def via_reference(scene, clamp, B, H, n):
    """The via term of a shape's seeded walks from the existing kernels on the MATERIALISED via points, computed once:
    cost (B,H) fp32 = the sum over a of the per-point costs by fp32 adds in ascending a (0 at t = H-1); fold (B,H,2) fp64 = L[t] + U[t-1]
    of the per-point fp32 gradients with the fp64 values of the fp32 weights; S its absolute counterpart; fold_swapped with alpha and
    beta exchanged."""
    key = (scene, clamp, B, H, n)
    if key not in _refs:
        h, _ = edges.variant(*scene)
        q = dev(inputs(scene[0], B, H)[0])
        pts = ops.interpolate_traj_via_points(q, n)
        c, g = ops.planar_cost_grad(h, pts.reshape(-1, 2), clamp=clamp)
        c, g = c.reshape(B, H - 1, n), g.reshape(B, H - 1, n, 2).double()
        acc = torch.zeros(B, H - 1, **TA)
        for a in range(n):
            acc = acc + c[:, :, a]
        cost = torch.zeros(B, H, **TA)
        cost[:, :H - 1] = acc
        alpha, beta = (w.double().reshape(1, 1, n, 1) for w in ops.via_point_weights(n, DEV))

        def fold(wl, wu, x):
            out = torch.zeros(B, H, 2, device=DEV, dtype=torch.float64)
            out[:, :H - 1] += (wl * x).sum(2)
            out[:, 1:] += (wu * x).sum(2)
            return out

        _refs[key] = dict(cost=cost, fold=host(fold(alpha, beta, g)), S=host(fold(alpha, beta, g.abs())), swapped=host(fold(beta, alpha, g)),
                          pts=pts)
    return _refs[key]


def via_call(h, q, qd, par, w_via, n, clamp, want_grad=True):
    dt, sigma, w, w_obj = par
    return ops.planar_traj_via_cost_grad(h, q, qd, dt, sigma, w, w_obj, w_via, n, clamp, want_grad=want_grad)


def via_plan(h, q, qd, par, w_via, n, clamp, lr=LR, pin=3, force=False):
    dt, sigma, w, w_obj = par
    plan = ops.PlanarAdamPlan(h, q, qd, dt, sigma, w, w_obj, clamp, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                              pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8), w_via=w_via, num_interpolation=n)
    if force:                               # the new entry point also where the plan would not bind it (w_via = 0)
        plan._bind(via=True)
    assert plan._fn.__name__ == ("trk_scene2d_traj_via_adam_steps" if force or (n > 0 and w_via != 0) else "trk_scene2d_traj_adam_steps")
    return plan


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", CASES)
def test_off_means_off(scene, clamp):
    h, _ = edges.variant(*scene)
    for k, (B, H) in enumerate(SHAPES):
        par = params_of(k)
        dt, sigma, w, w_obj = par
        q0, qd0 = inputs(scene[0], B, H)
        q, qd = dev(q0), dev(qd0)
        base = ops.planar_traj_cost_grad(h, q, qd, dt, sigma, w, w_obj, clamp)
        for n in N_INTERP:
            got = via_call(h, q, qd, par, 0.0, n, clamp)
            assert all(torch.equal(x, y) for x, y in zip(got, base)), (B, H, n)
        n = N_INTERP[k % len(N_INTERP)]
        for K in (1, 33):
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            via, plain = via_plan(h, qa, qda, par, 0.0, n, clamp, force=True), tp.plan_of(h, qb, qdb, par, clamp)
            assert torch.equal(via.step(K), plain.step(K)) and via.t == K
            for x, y, what in ((qa, qb, "q"), (qda, qdb, "qd"), (via.m, plain.m, "m"), (via.v, plain.v, "v")):
                assert torch.equal(x, y), (B, H, K, what)
    # without the keywords, and with only one of them, the plan binds what it bound before
    assert via_plan(h, q, qd, par, 0.0, 0, clamp)._fn.__name__ == "trk_scene2d_traj_adam_steps"
    assert via_plan(h, q, qd, par, 1.0, 0, clamp)._fn.__name__ == "trk_scene2d_traj_adam_steps"
    # H = 1 has no segment
    q1, qd1 = (dev(x) for x in inputs(scene[0], 300, 1))
    par = pt.PARAMS[0]
    base = ops.planar_traj_cost_grad(h, q1, qd1, par[0], par[1], par[2], par[3], clamp)
    assert all(torch.equal(x, y) for x, y in zip(via_call(h, q1, qd1, par, 1.0, 5, clamp), base))


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", CASES)
def test_the_via_term_alone(scene, clamp):
    """cost: bit-equal to the existing kernel's per-point costs added in ascending a.  gq: the kernel forms L and U by n fused
    multiply-adds each from 0, adds the two sums and folds them in with one fma, n + 2 roundings along either chain, each on a partial
    result no larger than S = sum_a alpha |g(v[t,a])| + sum_a beta |g(v[t-1,a])| -- within the (n + 3) 2^-24 S the bound allows."""
    h, _ = edges.variant(*scene)
    par = (0.08, 1.0, 0.0, 0.0)             # gp_weight = 0, w_obj = 0
    swap_rows = {n: 0 for n in N_INTERP if n >= 2}
    for B, H in SHAPES:
        q, qd = (dev(x) for x in inputs(scene[0], B, H))
        for n in N_INTERP:
            ref = via_reference(scene, clamp, B, H, n)
            cost, gq, gqd = via_call(h, q, qd, par, 1.0, n, clamp)
            assert torch.equal(cost, ref["cost"]), (B, H, n)
            assert not cost[:, H - 1].any() and not gqd.any(), (B, H, n)
            bound = (n + 3) * EPS * ref["S"]
            err = np.abs(host(gq).astype(np.float64) - ref["fold"])
            worst = float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0
            print(f"via alone {scene[0]} clamp={clamp} {B}x{H} n={n}: worst fold error / bound {worst:.3f}")
            assert (err <= bound).all(), (B, H, n)
            if n >= 2:                      # rows on which alpha and beta exchanged in the reference miss the same bound by more than 100x
                swap_rows[n] += int((np.abs(host(gq).astype(np.float64) - ref["swapped"]) > 100.0 * bound).any(-1).sum())
    print(f"via alone {scene[0]} clamp={clamp}: rows that expose a swapped fold, by n: {swap_rows}")
    assert all(v > 0 for v in swap_rows.values()), swap_rows     # the check has the power to see a swapped fold


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", pt.SCENES[:2], ids=lambda s: s[0])
@pytest.mark.parametrize("clamp", (False, True))
def test_via_cost_against_fp64(scene, clamp):
    """independent of the kernels: the via points formed in numpy fp32 (each product and the sum rounded once), the hinge of
    helpers.planar64 at them, summed in fp64"""
    h, a = edges.variant(*scene)
    par = (0.08, 1.0, 0.0, 0.0)
    for B, H in SHAPES:
        q0, qd0 = inputs(scene[0], B, H)
        for n in N_INTERP:
            alpha, beta = (host(w).reshape(1, 1, n, 1) for w in ops.via_point_weights(n, DEV))
            pts = (q0[:, :-1, None, :] * alpha).astype(np.float32) + (q0[:, 1:, None, :] * beta).astype(np.float32)
            assert pts.dtype == np.float32
            c64 = hp.planar64(a["objects"], pts.reshape(-1, 2), a["margin"], ws=a["ws"], grid=a["grid"], clamp=clamp, want_grad=False)[0]
            want = np.zeros((B, H))
            want[:, :H - 1] = c64.reshape(B, H - 1, n).sum(-1)
            cost = via_call(h, dev(q0), dev(qd0), par, 1.0, n, clamp, want_grad=False)[0]
            err, bound = np.abs(host(cost) - want).max(), pt.TOL_HINGE_COST * np.abs(want).max()
            print(f"via cost {scene[0]} clamp={clamp} {B}x{H} n={n}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (B, H, n)


# 4 ---------------------------------------------------------------------------------------------------------------------------
_prior = {}


def prior64(oracle, name, B, H, par):
    key = (name, B, H, par)
    if key not in _prior:
        dt, sigma, w, _ = par
        q, qd = (x.astype(np.float64) for x in inputs(name, B, H))
        _prior[key] = (oracle.gp_factor_cost(q, qd, dt, sigma, w, "f64"),) + tuple(oracle.gp_prior(q, qd, dt, sigma, w, "f64")[1:])
    return _prior[key]


@pytest.mark.parametrize("scene,clamp", CASES)
@pytest.mark.parametrize("par", pt.PARAMS)
@pytest.mark.parametrize("w_via", (1.0, 0.37))
def test_all_three_terms(scene, clamp, par, w_via, oracle_lib):
    """cost = fmaf(w_via, C, fmaf(w_obj, h, prior)) and gq likewise: against w_obj x the existing kernel's fp32 hinge at the way points
    + w_via x the via reference + the fp64 prior.  Roundings: those of test_the_via_term_alone (n + 3) and two more for the way-point
    term (its product inside the fma and that fma's result), each on a partial sum bounded by the sum of the three terms' magnitudes;
    the prior at TOL_PRIOR_COST / TOL_PRIOR_GRAD of its largest entry, as test_prior_half_against_fp64 applies them."""
    h, _ = edges.variant(*scene)
    dt, sigma, w, w_obj = par
    for B, H in SHAPES:
        q, qd = (dev(x) for x in inputs(scene[0], B, H))
        pf, pgq, pgqd = prior64(oracle_lib, scene[0], B, H, par)
        h0, g0 = ops.planar_cost_grad(h, q.reshape(-1, 2), clamp=clamp)
        h0, g0 = host(h0).reshape(B, H).astype(np.float64), host(g0).reshape(B, H, 2).astype(np.float64)
        for n in N_INTERP:
            ref = via_reference(scene, clamp, B, H, n)
            cost, gq, gqd = via_call(h, q, qd, par, w_via, n, clamp)
            only, none_q, none_qd = via_call(h, q, qd, par, w_via, n, clamp, want_grad=False)
            assert none_q is None and none_qd is None and torch.equal(only, cost)
            c_via = host(ref["cost"]).astype(np.float64)
            want = w_obj * h0 + w_via * c_via + pf
            bound = 2 * EPS * (np.abs(w_obj * h0) + np.abs(w_via * c_via) + np.abs(pf)) + pt.TOL_PRIOR_COST * np.abs(pf).max()
            err = np.abs(host(cost) - want)
            assert (err <= bound).all(), (B, H, n, float((err - bound).max()))
            want = w_obj * g0 + w_via * ref["fold"] + pgq
            bound = (n + 5) * EPS * (np.abs(w_obj * g0) + abs(w_via) * ref["S"] + np.abs(pgq)) + pt.TOL_PRIOR_GRAD * np.abs(pgq).max()
            err = np.abs(host(gq) - want)
            print(f"all {scene[0]} clamp={clamp} w_via={w_via} {B}x{H} n={n}: worst gq error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all(), (B, H, n, float((err - bound).max()))
            assert rel_err(host(gqd), pgqd) < pt.TOL_PRIOR_GRAD, (B, H, n)


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", CASES)
def test_one_adam_step_then_a_second(scene, clamp):
    h, _ = edges.variant(*scene)
    for k, ((B, H), n) in enumerate((s, n) for s in SHAPES for n in N_INTERP):
        par, w_via = params_of(k), (1.0, 0.37)[k % 2]
        q0, qd0 = inputs(scene[0], B, H)
        q, qd = dev(q0), dev(qd0)
        plan = via_plan(h, q, qd, par, w_via, n, clamp, pin=3)
        pinned = pt.pin_masks(3, B, H)
        state = lambda: np.concatenate([host(q), host(qd)], -1)
        x_prev, m_prev, v_prev = state(), host(plan.m).copy(), host(plan.v).copy()
        for step in (1, 2):
            c, gq, gqd = via_call(h, q, qd, par, w_via, n, clamp)
            g = np.concatenate([host(gq), host(gqd)], -1)
            assert torch.equal(plan.step(1), c) and plan.t == step
            x_new, m_new, v_new = state(), host(plan.m).copy(), host(plan.v).copy()
            tp.check_adam_step(step, x_prev, m_prev, v_prev, g, x_new, m_new, v_new, pinned)
            x_prev, m_prev, v_prev = x_new, m_new, v_new


@pytest.mark.parametrize("scene,clamp", CASES)
def test_grouping_of_iterations_does_not_matter(scene, clamp):
    h, _ = edges.variant(*scene)
    for k, ((B, H), n) in enumerate((s, n) for s in SHAPES for n in N_INTERP):
        par, w_via = params_of(k), (1.0, 0.37)[k % 2]
        q0, qd0 = inputs(scene[0], B, H)
        c0 = via_call(h, dev(q0), dev(qd0), par, w_via, n, clamp, want_grad=False)[0]
        for K in pt.GROUPINGS:
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            one, many = via_plan(h, qa, qda, par, w_via, n, clamp), via_plan(h, qb, qdb, par, w_via, n, clamp)
            assert torch.equal(one.step(K), c0)
            for _ in range(K):
                many.step(1)
            assert one.t == K and many.t == K
            for x, y, what in ((qa, qb, "q"), (qda, qdb, "qd"), (one.m, many.m, "m"), (one.v, many.v, "v")):
                assert torch.equal(x, y), (B, H, K, what, int((x != y).sum()))
            assert bool(torch.isfinite(qa).all() and torch.isfinite(qda).all())
        if H > 2:
            assert not torch.equal(qa, dev(q0))             # the iterations did move the trajectories


@pytest.mark.parametrize("scene,clamp", [(pt.SCENES[0], True), (pt.SCENES[1], False)])
def test_pins(scene, clamp):
    h, _ = edges.variant(*scene)
    B, H = 5, 63
    q0, qd0 = inputs(scene[0], B, H)
    x0 = np.concatenate([q0, qd0], -1)
    for pin in range(16):
        q, qd = dev(q0), dev(qd0)
        plan = via_plan(h, q, qd, pt.PARAMS[0], 1.0, 5, clamp, pin=pin)
        assert plan.pin == pin
        plan.step(33)
        x = np.concatenate([host(q), host(qd)], -1)
        held = pt.pin_masks(pin, B, H)
        assert np.array_equal(x[held].view(np.uint32), x0[held].view(np.uint32)), pin
        assert not host(plan.m)[held].any() and not host(plan.v)[held].any(), pin
        if pin == 0:
            assert (x[:, 0, :2] != x0[:, 0, :2]).any(-1).all() and (x[:, H - 1, :2] != x0[:, H - 1, :2]).any(-1).all()


def test_no_ops():
    h, _ = edges.variant(*pt.SCENES[0])
    par = pt.PARAMS[0]
    q0, qd0 = inputs("gridposed", 5, 63)
    # lr = 0 evaluates: the cost is written, nothing else
    q, qd = dev(q0), dev(qd0)
    plan = via_plan(h, q, qd, par, 1.0, 5, True, lr=0.0)
    plan.m.fill_(0.25); plan.v.fill_(0.5); plan.cost.fill_(float("nan"))
    cost = plan.step(7)
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((plan.m == 0.25).all()) and bool((plan.v == 0.5).all())
    assert torch.equal(cost, via_call(h, q, qd, par, 1.0, 5, True, want_grad=False)[0]) and plan.t == 0
    assert not torch.equal(cost, ops.planar_traj_cost_grad(h, q, qd, par[0], par[1], par[2], par[3], True, want_grad=False)[0])
    # an empty batch returns at once
    e = torch.empty(0, 63, 2, device=DEV)
    assert via_plan(h, e, e.clone(), par, 1.0, 5, True).step(3).shape == (0, 63)
    c, gq, gqd = via_call(h, e, e.clone(), par, 1.0, 5, True)
    assert c.shape == (0, 63) and gq.shape == (0, 63, 2) and gqd.shape == (0, 63, 2)
    # one layout: both calls stop at 256 samples, by name
    big = torch.zeros(1, 257, 2, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        via_plan(h, big, big.clone(), par, 1.0, 5, True)
    with pytest.raises(NotImplementedError, match="256"):
        via_call(h, big, big.clone(), par, 1.0, 5, True)
    with pytest.raises(ValueError):
        via_call(h, q, qd, par, 1.0, 0, True)


# 6 ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = 12345.5


def off_boundary(shape):
    """a view 8 bytes off a 16-byte boundary inside a buffer of sentinels -> (view, buffer, the view's slice of the buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), SENTINEL, **TA)
    assert buf.data_ptr() % 16 == 0
    view = buf[2:2 + n].view(shape)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view, buf, slice(2, 2 + n)


def sentinels_intact(buf, sl):
    return bool((buf[:sl.start] == SENTINEL).all() and (buf[sl.stop:] == SENTINEL).all())


@pytest.mark.parametrize("B,H", [(4, 64), (5, 63)])
@pytest.mark.parametrize("scene,clamp", [(pt.SCENES[0], True), (pt.SCENES[2], False)])
def test_a_non_finite_trajectory_stays_alone(scene, clamp, B, H):
    h, _ = edges.variant(*scene)
    par, w_via, n = pt.PARAMS[0], 1.0, 5
    q0, qd0 = inputs(scene[0], B, H)
    bad = B // 2
    others = [b for b in range(B) if b != bad]
    obj, _keep = ops._planar_via_objective(*par, clamp, w_via, n, DEV)
    results = []
    for poison in (False, True):
        (q, qb, qs), (qd, qdb, qds) = off_boundary((B, H, 2)), off_boundary((B, H, 2))
        (cost, cb, cs), (gq, gb, gs), (gqd, gdb, gds) = off_boundary((B, H)), off_boundary((B, H, 2)), off_boundary((B, H, 2))
        q.copy_(dev(q0)); qd.copy_(dev(qd0))
        if poison:
            q[bad] = float("nan")
        rc = _lib.lib().trk_scene2d_traj_via_cost_grad(h._h, C.byref(obj), q.data_ptr(), qd.data_ptr(), B, H, cost.data_ptr(), gq.data_ptr(),
                                                       gqd.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == _abi.TRK_OK
        first = [t.clone() for t in (cost, gq, gqd)]
        plan = via_plan(h, q, qd, par, w_via, n, clamp, pin=0)
        plan.step(3)
        torch.cuda.synchronize()
        for buf, sl in ((qb, qs), (qdb, qds), (cb, cs), (gb, gs), (gdb, gds)):
            assert sentinels_intact(buf, sl)
        results.append(first + [q.clone(), qd.clone(), plan.m.clone(), plan.v.clone(), plan.cost.clone()])
    for clean, dirty, what in zip(results[0], results[1], ("cost", "gq", "gqd", "q", "qd", "m", "v", "plan.cost")):
        assert torch.equal(clean[others], dirty[others]), what
        assert bool(torch.isfinite(clean).all()), what
    assert bool(torch.isnan(results[1][0][bad]).any()) and not torch.equal(results[0][3], dev(q0))


# 7 ---------------------------------------------------------------------------------------------------------------------------
def planar_task(env_name):
    return tra.PlanningTask(env=getattr(tra, env_name)(tensor_args=TA), robot=tra.RobotPointMass(tensor_args=TA), obstacle_cutoff_margin=0.02,
                            clamp_sdf=True, tensor_args=TA)


@pytest.mark.parametrize("env_name", ["EnvDense2D", "EnvNarrowPassageDense2D"])
def test_through_the_task_and_a_captured_graph(env_name):
    task = planar_task(env_name)
    lo, hi = (host(v) for v in task.env.limits)
    q0, qd0 = pt.random_walks((lo, hi), 9, 64, seed=7)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    via_task = task.trajectory_optimizer(qa, qda, 5.0 / 64, 1.0, w_obj=20.0, lr=LR, w_via=4.0, num_interpolation=5, pin_goal_vel=True)
    scene, clamp = task._planar_handles(DEV)
    direct = ops.PlanarAdamPlan(scene, qb, qdb, 5.0 / 64, 1.0, 1.0, 20.0, clamp, LR, pin_goal_vel=True, w_via=4.0, num_interpolation=5)
    assert clamp and via_task.pin == 11 and via_task._fn.__name__ == "trk_scene2d_traj_via_adam_steps"
    for n in (1, 40):
        assert torch.equal(via_task.step(n), direct.step(n))
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(via_task.m, direct.m) and torch.equal(via_task.v, direct.v)
    assert via_task.t == 41 and not torch.equal(qa, dev(q0))
    plain = task.trajectory_optimizer(dev(q0), dev(qd0), 5.0 / 64, 1.0, w_obj=20.0, lr=LR, pin_goal_vel=True)
    plain.step(41)
    assert not torch.equal(plain.q, qa)                     # the via term did steer the trajectories elsewhere
    # a captured step(32) carries the bias terms of its iterations by value: two replays are two eager steps from the same counter
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        via_task.step(32)
    for _ in range(2):
        graph.replay()
        direct.t = 41
        direct.step(32)
    torch.cuda.synchronize()
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(via_task.m, direct.m) and torch.equal(via_task.v, direct.v)
    assert torch.equal(via_task.cost, direct.cost)


def test_fused_example_with_the_via_term_frees_trajectories():
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("plan_point_mass_2d", Path(hp.ROOT) / "examples" / "plan_point_mass_2d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after = mod.main(batch=128, horizon=64, iters=100, verbose=False, fused=True, via_cost=5)
    _, plain = mod.main(batch=128, horizon=64, iters=100, verbose=False, fused=True)
    print(f"fused example, 128 x 64, 100 iterations: free fraction {before:.3f} -> {after:.3f} with 5 via points per segment in the "
          f"objective, -> {plain:.3f} without")
    assert after > before

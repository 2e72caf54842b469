"""The 2-D point mass's trajectory objective and its in-kernel Adam loop (csrc/trk_planar.hip: k_planar_traj_cost,
k_planar_traj_adam) on the synthetic scenes of tests/golden/pointmass2d_synth_*.npz.

The hinge half is pinned to the existing kernel bit for bit (which carries over what tests/test_gpu_planar2d_edges.py establishes, kinks
included), the prior half to the fp64 oracle at test_gp_prior_vs_fp64_oracle's tolerances, the Adam update to its formula in fp64 on the
kernel's own moments, and the grouping of iterations into launches and calls to bit equality.  Cases and bounds: planar_traj_helpers."""
import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import planar_traj_helpers as pt
import test_gpu_planar2d_edges as edges
from helpers import rel_err
from torch_robotics_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
CASES = [(s, clamp) for s in pt.SCENES for clamp in (False, True)]
LR = 5e-3
_inputs = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def inputs(name, B, H):
    """the seeded random walks of a scene and a shape, computed once and never written to"""
    if (name, B, H) not in _inputs:
        limits = edges.fixture(name)[1]["limits"]
        _inputs[(name, B, H)] = pt.random_walks(limits, B, H, seed=1000 * B + H)
    return _inputs[(name, B, H)]


def params_of(k):
    return pt.PARAMS[k % len(pt.PARAMS)]


def plan_of(h, q, qd, par, clamp, lr=LR, pin=3):
    dt, sigma, w, w_obj = par
    return ops.PlanarAdamPlan(h, q, qd, dt, sigma, w, w_obj, clamp, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                              pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8))


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", CASES)
def test_hinge_half_is_the_existing_kernel(scene, clamp):
    h, _ = edges.variant(*scene)
    for k, (B, H) in enumerate(pt.SHAPES):
        q, qd = (dev(x) for x in inputs(scene[0], B, H))
        dt, sigma, _, _ = params_of(k)
        cost, gq, gqd = ops.planar_traj_cost_grad(h, q, qd, dt, sigma, gp_weight=0.0, w_obj=1.0, clamp=clamp)
        c0, g0 = ops.planar_cost_grad(h, q.reshape(-1, 2), clamp=clamp)
        assert cost.shape == (B, H) and gq.shape == (B, H, 2) and gqd.shape == (B, H, 2)
        assert torch.equal(cost.reshape(-1), c0) and torch.equal(gq.reshape(-1, 2), g0), (B, H)
        assert not gqd.any(), (B, H)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", pt.PARAMS)
def test_prior_half_against_fp64(par, oracle_lib):
    h, a = edges.variant(*pt.SCENES[0])
    dt, sigma, w, _ = par
    for B, H in pt.SHAPES:
        q, qd = inputs("gridposed", B, H)
        ref = pt.objective64(oracle_lib, a, q, qd, dt, sigma, w, 0.0, False)
        cost, gq, gqd = ops.planar_traj_cost_grad(h, dev(q), dev(qd), dt, sigma, gp_weight=w, w_obj=0.0, clamp=False)
        if H == 1:
            assert not cost.any() and not gq.any() and not gqd.any()
            continue
        print(f"prior {B}x{H}: total {rel_err(host(cost).astype(np.float64).sum(1), ref['prior_total']):.2e} factor "
              f"{rel_err(host(cost), ref['prior']):.2e} gq {rel_err(host(gq), ref['prior_gq']):.2e} gqd {rel_err(host(gqd), ref['prior_gqd']):.2e}")
        assert rel_err(host(cost).astype(np.float64).sum(1), ref["prior_total"]) < pt.TOL_PRIOR_COST
        assert rel_err(host(cost), ref["prior"]) < pt.TOL_PRIOR_COST
        assert rel_err(host(gq), ref["prior_gq"]) < pt.TOL_PRIOR_GRAD and rel_err(host(gqd), ref["prior_gqd"]) < pt.TOL_PRIOR_GRAD


# 3 ---------------------------------------------------------------------------------------------------------------------------
def decided_rows(scene, a, q, s64, clamp):
    if not clamp:
        return np.ones(q.shape[0] * q.shape[1], bool)
    band = 2.0 * float(edges.fixture(scene[0])[0]["band_measured"])
    return hp.planar_hinge_decided(s64, q.reshape(-1, 2), a["ws"], float(a["margin"]), band)


@pytest.mark.parametrize("scene,clamp", CASES)
@pytest.mark.parametrize("par", pt.PARAMS)
def test_both_halves_against_fp64(scene, clamp, par, oracle_lib):
    h, a = edges.variant(*scene)
    dt, sigma, w, w_obj = par
    for B, H in pt.SHAPES:
        q, qd = inputs(scene[0], B, H)
        n = B * H
        ref = pt.objective64(oracle_lib, a, q, qd, dt, sigma, w, w_obj, clamp)
        cost, gq, gqd = ops.planar_traj_cost_grad(h, dev(q), dev(qd), dt, sigma, gp_weight=w, w_obj=w_obj, clamp=clamp)
        only, none_q, none_qd = ops.planar_traj_cost_grad(h, dev(q), dev(qd), dt, sigma, gp_weight=w, w_obj=w_obj, clamp=clamp, want_grad=False)
        assert none_q is None and none_qd is None and torch.equal(only, cost)
        err, bound = np.abs(host(cost) - ref["cost"]).max(), pt.cost_bound(ref, w_obj)
        print(f"both {scene[0]} clamp={clamp} {B}x{H}: cost err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (B, H)
        dec = decided_rows(scene, a, q, ref["sdf"], clamp)
        assert 2 * int(dec.sum()) >= n, (B, H, int(dec.sum()))            # at least half of every batch is judged here
        got, want = host(gq).reshape(-1, 2)[dec], ref["gq"].reshape(-1, 2)[dec]
        bad = hp.planar_bad_rows(got, want) if np.abs(want).max() > 0 else np.abs(got).max(-1) > 0
        assert bad.sum() <= n // 10000, (B, H, int(bad.sum()), np.flatnonzero(bad)[:8])
        if H > 1:
            assert rel_err(host(gqd), ref["gqd"]) < pt.TOL_PRIOR_GRAD


# 4 ---------------------------------------------------------------------------------------------------------------------------
def check_adam_step(step, x0, m0, v0, g, x1, m1, v1, pinned):
    """one iteration: the moments against the validated gradient, the new values against the update formula in fp64 on the returned
    moments and the fp32 bias terms"""
    g = np.where(pinned, 0.0, g.astype(np.float64))
    x0, m0, v0, x1, m1, v1 = (t.astype(np.float64) for t in (x0, m0, v0, x1, m1, v1))
    gmax = max(1e-30, np.abs(g).max())
    # m1 = 0.9 m0 + 0.1 g: planar_bad_rows' bound on g, scaled by 0.1, plus the roundings of the fma and the product
    assert (np.abs(m1 - (0.9 * m0 + 0.1 * g)) <= 0.1 * (hp.GRAD_RTOL * np.abs(g) + hp.GRAD_ATOL * gmax) + 2.0 ** -22 * np.abs(m1)).all()
    # v1 = 0.999 v0 + 0.001 g^2: twice the relative part on g^2
    assert (np.abs(v1 - (0.999 * v0 + 0.001 * g * g)) <= 0.001 * 2.0 * hp.GRAD_RTOL * g * g + 2.0 ** -22 * np.abs(v1)).all()
    bc1, rs = ops.planar_adam_bias_terms(step)
    upd = (float(np.float32(LR)) / bc1) * m1 / (np.sqrt(v1) * rs + 1e-8)            # lr as the ABI carries it: a float
    bound = 0.5 * np.spacing(np.abs(x1).astype(np.float32)).astype(np.float64) + 2.0 * pt.ADAM_ROUNDINGS * 2.0 ** -24 * np.abs(upd)
    err = np.abs(x1 - (x0 - upd))
    print(f"adam step {step}: worst update error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(x1[pinned], x0[pinned]) and not m1[pinned].any() and not v1[pinned].any()


@pytest.mark.parametrize("scene,clamp", CASES)
def test_one_adam_step_then_a_second(scene, clamp):
    h, _ = edges.variant(*scene)
    for k, (B, H) in enumerate(pt.SHAPES):
        par = params_of(k)
        dt, sigma, w, w_obj = par
        q0, qd0 = inputs(scene[0], B, H)
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, q, qd, par, clamp, pin=3)
        pinned = pt.pin_masks(3, B, H)
        state = lambda: np.concatenate([host(q), host(qd)], -1)
        x_prev, m_prev, v_prev = state(), host(plan.m).copy(), host(plan.v).copy()
        assert not m_prev.any() and not v_prev.any()
        for step in (1, 2):
            _, gq, gqd = ops.planar_traj_cost_grad(h, q, qd, dt, sigma, w, w_obj, clamp)
            g = np.concatenate([host(gq), host(gqd)], -1)
            plan.step(1)
            assert plan.t == step
            x_new, m_new, v_new = state(), host(plan.m).copy(), host(plan.v).copy()
            check_adam_step(step, x_prev, m_prev, v_prev, g, x_new, m_new, v_new, pinned)
            x_prev, m_prev, v_prev = x_new, m_new, v_new


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", CASES)
def test_grouping_of_iterations_does_not_matter(scene, clamp, oracle_lib):
    h, a = edges.variant(*scene)
    for k, (B, H) in enumerate(pt.SHAPES):
        par = params_of(k)
        dt, sigma, w, w_obj = par
        q0, qd0 = inputs(scene[0], B, H)
        c0 = ops.planar_traj_cost_grad(h, dev(q0), dev(qd0), dt, sigma, w, w_obj, clamp, want_grad=False)[0]
        bound = pt.cost_bound(pt.objective64(oracle_lib, a, q0, qd0, dt, sigma, w, w_obj, clamp), w_obj)
        for K in pt.GROUPINGS:
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            one, many = plan_of(h, qa, qda, par, clamp), plan_of(h, qb, qdb, par, clamp)
            cost = one.step(K).clone()
            for _ in range(K):
                many.step(1)
            assert one.t == K and many.t == K
            for x, y, what in ((qa, qb, "q"), (qda, qdb, "qd"), (one.m, many.m, "m"), (one.v, many.v, "v")):
                assert torch.equal(x, y), (B, H, K, what, int((x != y).sum()))
            assert bool(torch.isfinite(qa).all() and torch.isfinite(qda).all())
            assert float((cost - c0).abs().max()) <= bound, (B, H, K)
        if H > 2:
            assert not torch.equal(qa, dev(q0))             # the iterations did move the trajectories


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp", [(pt.SCENES[0], True), (pt.SCENES[1], False)])
def test_pins(scene, clamp):
    h, _ = edges.variant(*scene)
    B, H = 5, 63
    q0, qd0 = inputs(scene[0], B, H)
    x0 = np.concatenate([q0, qd0], -1)
    for pin in range(16):
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, q, qd, pt.PARAMS[0], clamp, pin=pin)
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
    dt, sigma, w, w_obj = par
    q0, qd0 = inputs("gridposed", 5, 63)
    # lr = 0 evaluates: the cost is written, nothing else
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, q, qd, par, True, lr=0.0)
    plan.m.fill_(0.25); plan.v.fill_(0.5); plan.cost.fill_(float("nan"))
    cost = plan.step(7)
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((plan.m == 0.25).all()) and bool((plan.v == 0.5).all())
    assert torch.equal(cost, ops.planar_traj_cost_grad(h, q, qd, dt, sigma, w, w_obj, True, want_grad=False)[0]) and plan.t == 0
    # an empty batch returns at once
    e = torch.empty(0, 63, 2, device=DEV)
    plan = plan_of(h, e, e.clone(), par, True)
    assert plan.step(3).shape == (0, 63)
    c, gq, gqd = ops.planar_traj_cost_grad(h, e, e.clone(), dt, sigma)
    assert c.shape == (0, 63) and gq.shape == (0, 63, 2) and gqd.shape == (0, 63, 2)
    # H = 1 has no factor: with the prior on, the step is the hinge-only step
    q1, qd1 = inputs("gridposed", 300, 1)
    qa, qda, qb, qdb = dev(q1), dev(qd1), dev(q1), dev(qd1)
    on, off = plan_of(h, qa, qda, par, True, pin=0), plan_of(h, qb, qdb, (dt, sigma, 0.0, w_obj), True, pin=0)
    on.step(5); off.step(5)
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(on.m, off.m) and torch.equal(on.v, off.v)
    assert not torch.equal(qa, dev(q1)) and torch.equal(qda, dev(qd1))
    # beyond the persistent kernel's horizon: refused by name, while the one-launch objective serves it
    big = torch.zeros(1, 257, 2, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        plan_of(h, big, big.clone(), par, True)
    assert ops.planar_traj_cost_grad(h, big, big.clone(), dt, sigma)[0].shape == (1, 257)
    with pytest.raises(ValueError):
        ops.planar_traj_cost_grad(h, big, big[:, :5].clone(), dt, sigma)


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["EnvDense2D", "EnvNarrowPassageDense2D"])
def test_through_the_task(env_name):
    task = tra.PlanningTask(env=getattr(tra, env_name)(tensor_args=TA), robot=tra.RobotPointMass(tensor_args=TA), obstacle_cutoff_margin=0.02,
                            clamp_sdf=True, tensor_args=TA)
    lo, hi = (host(v) for v in task.env.limits)
    q0, qd0 = pt.random_walks((lo, hi), 9, 64, seed=7)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    via_task = task.trajectory_optimizer(qa, qda, 5.0 / 64, 1.0, w_obj=20.0, lr=LR, pin_goal_vel=True)
    scene, clamp = task._planar_handles(DEV)
    direct = ops.PlanarAdamPlan(scene, qb, qdb, 5.0 / 64, 1.0, 1.0, 20.0, clamp, LR, pin_goal_vel=True)
    assert clamp and via_task.pin == 11
    for n in (1, 40):
        assert torch.equal(via_task.step(n), direct.step(n))
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(via_task.m, direct.m) and torch.equal(via_task.v, direct.v)
    assert via_task.t == 41 and not torch.equal(qa, dev(q0))


def test_fused_example_frees_trajectories():
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("plan_point_mass_2d", Path(hp.ROOT) / "examples" / "plan_point_mass_2d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after = mod.main(batch=128, horizon=64, iters=100, verbose=False, fused=True)
    print(f"fused example, 128 x 64, 100 iterations: free fraction {before:.3f} -> {after:.3f}")
    assert after > before

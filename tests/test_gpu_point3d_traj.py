"""The 3-D point mass's trajectory objective and its in-kernel Adam loop (csrc/trk_point3d.hip: k_point3d_traj) behind
trk_point3d_traj_cost_grad and trk_point3d_traj_adam_steps, on the three scenes of point3d_traj_helpers: EnvSpheres3D's ten equal
spheres (the paired ranking path of scene_min_sdf), unequal spheres with a rotated rounded-box object, and a small voxel grid next to an
analytic sphere -- each with the workspace box, with clamp off and on.

The hinge half is pinned to trk_cost_fields bit for bit and to the reference's recorded 3-D point mass; the prior half, the whole
objective and the via term are held to the fp64 reference objective64 (validated on the CPU: tests/test_point3d_traj_cpu.py); the Adam
update to its formula in fp64 on the kernel's own moments; the grouping of iterations, the two exchanges (DPP and LDS), the pins, the
no-ops, the buffers' edges and the isolation of a non-finite trajectory to bit equality; then the route through the task, a captured
graph and the example.  Cases and bounds: point3d_traj_helpers, planar_traj_helpers."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import point3d_traj_helpers as p3
import test_gpu_planar_traj as tp
from helpers import rel_err
from torch_robotics_amd import _abi, _lib, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
LR = tp.LR                                  # check_adam_step forms the update with it
FIELDS = p3.FIELD_OBJECTS | p3.FIELD_WS
N_INTERP = (1, 2, 5)
TOL_C = 1e-5                                # tests/test_gpu_api.py, the recorded 3-D point mass
# (dt, sigma, gp_weight), (w_obj, w_ws): both PARAMS of planar_traj_helpers with their w_obj, and weights that are neither 0 nor 1
OBJECTIVES = [(p3.PARAMS[0][:3], (p3.PARAMS[0][3], 1.0)), (p3.PARAMS[1][:3], (p3.PARAMS[1][3], 1.0)), (p3.PARAMS[0][:3], p3.WEIGHTS)]
_handles = {}


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)          # a copy: the cached walks are read-only


def host(t):
    return t.detach().cpu().numpy()


def handle(name, clamp):
    if (name, clamp) not in _handles:
        _handles[(name, clamp)] = ops.CostHandle(p3.spec_of(name, clamp), DEV)
    return _handles[(name, clamp)]


def call(cm, q, qd, gp, w, via=None, want_grad=True):
    dt, sigma, gw = gp
    w_via, n = via if via is not None else (0.0, 0)
    return ops.point3d_traj_cost_grad(cm, (0.0, w[0], w[1], 0.0), q, qd, dt, sigma, gw, w_via=w_via, num_interpolation=n, want_grad=want_grad)


def plan_of(cm, q, qd, gp, w, via=None, lr=LR, pin=3):
    dt, sigma, gw = gp
    w_via, n = via if via is not None else (0.0, 0)
    plan = ops.Point3DAdamPlan(cm, (0.0, w[0], w[1], 0.0), q, qd, dt, sigma, gw, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                               pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8), w_via=w_via, num_interpolation=n)
    assert plan._fn.__name__ == "trk_point3d_traj_adam_steps" and (plan._via is not None) == (n > 0 and w_via != 0)
    return plan


def objective_of(k):
    return OBJECTIVES[k % len(OBJECTIVES)]


def judged_rows(oracle, name, clamp, q, n=0):
    """(B, H) bool: the rows of a case that are compared with the fp64 reference.  With clamp on, those whose own point -- and, with a
    via term, the via points of the segments before and after -- the fp64 hinge decides by more than CLAMP_BAND in both fields; in the
    grid scene, those whose points all lie FACE_BAND off the faces of the grid's cells (either side of a face is another cost)."""
    B, H, _ = q.shape

    def rows(pts):
        ok = p3.off_faces(name, pts)
        if clamp:
            ok &= p3.decided(p3.raw_fields(oracle, name, pts))
        return ok

    keep = rows(q.reshape(-1, 3)).reshape(B, H)
    if n > 0 and H > 1:
        seg = rows(p3.via_points(q, n).reshape(-1, 3)).reshape(B, H - 1, n).all(-1)
        keep[:, :H - 1] &= seg
        keep[:, 1:] &= seg
    return keep


def oracle_grad_of(oracle, spec, q, qd, gp, w, via):
    """oracle_grad for helpers.grad_close_kinks over the rows of q: d objective / d q[b,t] of the fp64 reference with q[b,t] moved to each
    probe (the row is found by its distance to the probes' centre; its trajectory is evaluated whole, so the prior's and the via term's
    shares move with it)"""
    flat = q.reshape(-1, 3).astype(np.float64)
    H = q.shape[1]

    def grad(probes):
        r = int(np.argmin(np.abs(flat - probes.mean(0)).max(-1)))
        b, t = divmod(r, H)
        out = []
        for p in probes:
            qq = q[b:b + 1].copy()
            qq[0, t] = p.astype(np.float32)
            out.append(p3.objective64(oracle, spec, qq, qd[b:b + 1], *gp, *w, via=via)["gq"][0, t])
        return np.stack(out)

    return grad


def check_against_fp64(oracle, name, clamp, gp, w, via, pooled):
    """one scene and objective over the ten shapes: cost within cost_bound, gq through grad_close_kinks, gqd against the prior's, all on
    the judged rows; want_grad=False gives the same cost bits"""
    cm, spec = handle(name, clamp), p3.spec_of(name, clamp)
    for B, H in p3.SHAPES:
        q, qd = p3.walks(name, B, H)
        ref = p3.objective64(oracle, spec, q, qd, *gp, *w, via=via)
        cost, gq, gqd = call(cm, dev(q), dev(qd), gp, w, via)
        only, none_q, none_qd = call(cm, dev(q), dev(qd), gp, w, via, want_grad=False)
        assert none_q is None and none_qd is None and torch.equal(only, cost), (B, H)
        keep = judged_rows(oracle, name, clamp, q, via[1] if via else 0)
        pooled[0] += int(keep.sum()); pooled[1] += B * H
        if not keep.any():
            continue
        err, bound = np.abs(host(cost) - ref["cost"])[keep].max(), p3.cost_bound(ref)
        print(f"{name} clamp={clamp} via={via} {B}x{H}: {int(keep.sum())} of {B * H} rows judged, cost err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (B, H)
        if not ref["gq"][keep].any():               # nothing to scale a bound with (one free sample, no prior factor): zero is zero
            assert not gq[dev(keep)].any(), (B, H)
        else:
            assert hp.grad_close_kinks(host(gq)[keep], ref["gq"][keep], q[keep], oracle_grad_of(oracle, spec, q, qd, gp, w, via)), (B, H)
        if H > 1 and gp[2] != 0.0:
            assert rel_err(host(gqd), ref["gqd"]) < p3.TOL_PRIOR_GRAD, (B, H)
        else:
            assert not gqd.any(), (B, H)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
def test_hinge_half_is_the_existing_kernel(name, clamp):
    cm = handle(name, clamp)
    for k, (B, H) in enumerate(p3.SHAPES):
        q, qd = (dev(x) for x in p3.walks(name, B, H))
        dt, sigma, _ = objective_of(k)[0]
        cost, gq, gqd = call(cm, q, qd, (dt, sigma, 0.0), (1.0, 1.0))
        c0, g0 = ops.cost_fields(cm, FIELDS, q.reshape(-1, 1, 3), want_grad=True)
        assert cost.shape == (B, H) and gq.shape == (B, H, 3) and gqd.shape == (B, H, 3)
        assert torch.equal(cost.reshape(-1), c0) and torch.equal(gq.reshape(-1, 1, 3), g0), (B, H)
        assert not gqd.any(), (B, H)


def test_hinge_half_on_the_recorded_point_mass():
    g = hp.gold("pointmass3d")
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=tra.RobotPointMass3D(tensor_args=TA),
                            obstacle_cutoff_margin=float(g["cutoff"]), tensor_args=TA)
    _, cm = task._fused_handles(DEV)
    q = dev(g["q"])
    cost, gq, gqd = call(cm, q, torch.zeros_like(q), (0.08, 1.0, 0.0), (1.0, 1.0))
    assert cost.shape == (6, 16) and rel_err(host(cost), g["cost"]) < TOL_C
    assert hp.grad_close(host(gq), g["gq"]) and not gqd.any()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", p3.PARAMS)
def test_prior_half_against_fp64(par, oracle_lib):
    cm, spec = handle("posed", False), p3.spec_of("posed", False)
    gp = par[:3]
    for B, H in p3.SHAPES:
        q, qd = p3.walks("posed", B, H)
        ref = p3.objective64(oracle_lib, spec, q, qd, *gp, 0.0, 0.0)
        cost, gq, gqd = call(cm, dev(q), dev(qd), gp, (0.0, 0.0))
        if H == 1:
            assert not cost.any() and not gq.any() and not gqd.any()
            continue
        print(f"prior {B}x{H}: total {rel_err(host(cost).astype(np.float64).sum(1), ref['prior_total']):.2e} factor "
              f"{rel_err(host(cost), ref['prior']):.2e} gq {rel_err(host(gq), ref['prior_gq']):.2e} gqd {rel_err(host(gqd), ref['prior_gqd']):.2e}")
        assert rel_err(host(cost).astype(np.float64).sum(1), ref["prior_total"]) < p3.TOL_PRIOR_COST
        assert rel_err(host(cost), ref["prior"]) < p3.TOL_PRIOR_COST and not cost[:, H - 1].any()
        assert rel_err(host(gq), ref["prior_gq"]) < p3.TOL_PRIOR_GRAD and rel_err(host(gqd), ref["prior_gqd"]) < p3.TOL_PRIOR_GRAD


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
@pytest.mark.parametrize("objective", OBJECTIVES, ids=("params0", "params1", "weights"))
def test_whole_objective_against_fp64(name, clamp, objective, oracle_lib):
    pooled = [0, 0]
    check_against_fp64(oracle_lib, name, clamp, objective[0], objective[1], None, pooled)
    print(f"{name} clamp={clamp}: {pooled[0]} of {pooled[1]} rows judged")
    assert pooled[0] >= 0.5 * pooled[1]


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
def test_via_off_means_off(name, clamp):
    cm = handle(name, clamp)
    for k, (B, H) in enumerate(p3.SHAPES):
        gp, w = objective_of(k)
        q0, qd0 = p3.walks(name, B, H)
        q, qd = dev(q0), dev(qd0)
        base = call(cm, q, qd, gp, w)
        for via in ((0.0, 5), (1.0, 0)):
            assert all(torch.equal(x, y) for x, y in zip(call(cm, q, qd, gp, w, via), base)), (B, H, via)
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            off, plain = plan_of(cm, qa, qda, gp, w, via), plan_of(cm, qb, qdb, gp, w)
            assert torch.equal(off.step(33), plain.step(33)) and off.t == 33
            for x, y, what in ((qa, qb, "q"), (qda, qdb, "qd"), (off.m, plain.m, "m"), (off.v, plain.v, "v")):
                assert torch.equal(x, y), (B, H, via, what)
    # H = 1 has no segment: the via form itself gives the plain bits
    q1, qd1 = (dev(x) for x in p3.walks(name, 300, 1))
    gp, w = OBJECTIVES[0]
    assert all(torch.equal(x, y) for x, y in zip(call(cm, q1, qd1, gp, w, (1.0, 5)), call(cm, q1, qd1, gp, w)))


@pytest.mark.parametrize("name,clamp", p3.CASES)
def test_the_via_term_against_fp64(name, clamp, oracle_lib):
    """the term alone (no prior) and all terms together, H = 1 and H = 2 among the shapes"""
    pooled = [0, 0]
    for k, n in enumerate(N_INTERP):
        gp, w = objective_of(k)
        check_against_fp64(oracle_lib, name, clamp, (gp[0], gp[1], 0.0), w, (1.0, n), pooled)
        check_against_fp64(oracle_lib, name, clamp, gp, w, (0.37, n), pooled)
    print(f"{name} clamp={clamp}: {pooled[0]} of {pooled[1]} rows judged")
    assert pooled[0] >= 0.5 * pooled[1]
    # the via term is there: the cost differs from the plain one where a segment's via points are in collision
    cm = handle(name, clamp)
    q, qd = (dev(x) for x in p3.walks(name, 37, 64))
    gp, w = OBJECTIVES[0]
    assert not torch.equal(call(cm, q, qd, gp, w, (1.0, 5))[0], call(cm, q, qd, gp, w)[0])


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
@pytest.mark.parametrize("with_via", (False, True), ids=("plain", "via"))
def test_one_adam_step_then_a_second(name, clamp, with_via):
    cm = handle(name, clamp)
    for k, (B, H) in enumerate(p3.SHAPES):
        gp, w = objective_of(k)
        via = ((1.0, 0.37)[k % 2], N_INTERP[k % 3]) if with_via else None
        q0, qd0 = p3.walks(name, B, H)
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(cm, q, qd, gp, w, via, pin=3)
        pinned = p3.pin_masks(3, B, H)
        state = lambda: np.concatenate([host(q), host(qd)], -1)
        x_prev, m_prev, v_prev = state(), host(plan.m).copy(), host(plan.v).copy()
        assert not m_prev.any() and not v_prev.any()
        for step in (1, 2):
            c, gq, gqd = call(cm, q, qd, gp, w, via)
            g = np.concatenate([host(gq), host(gqd)], -1)
            assert torch.equal(plan.step(1), c) and plan.t == step          # the loop's cost is the evaluation's, bit for bit
            x_new, m_new, v_new = state(), host(plan.m).copy(), host(plan.v).copy()
            tp.check_adam_step(step, x_prev, m_prev, v_prev, g, x_new, m_new, v_new, pinned)
            x_prev, m_prev, v_prev = x_new, m_new, v_new


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
@pytest.mark.parametrize("with_via", (False, True), ids=("plain", "via"))
def test_grouping_of_iterations_does_not_matter(name, clamp, with_via):
    cm = handle(name, clamp)
    for k, (B, H) in enumerate(p3.SHAPES):
        gp, w = objective_of(k)
        via = ((1.0, 0.37)[k % 2], N_INTERP[k % 3]) if with_via else None
        q0, qd0 = p3.walks(name, B, H)
        c0 = call(cm, dev(q0), dev(qd0), gp, w, via, want_grad=False)[0]
        for K in p3.GROUPINGS:
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            one, many = plan_of(cm, qa, qda, gp, w, via), plan_of(cm, qb, qdb, gp, w, via)
            assert torch.equal(one.step(K), c0)
            for _ in range(K):
                many.step(1)
            assert one.t == K and many.t == K
            for x, y, what in ((qa, qb, "q"), (qda, qdb, "qd"), (one.m, many.m, "m"), (one.v, many.v, "v")):
                assert torch.equal(x, y), (B, H, K, what, int((x != y).sum()))
            assert bool(torch.isfinite(qa).all() and torch.isfinite(qda).all())
        if H > 2:
            assert not torch.equal(qa, dev(q0))             # the iterations did move the trajectories


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", p3.CASES)
@pytest.mark.parametrize("B", (4, 37))
def test_both_transports_agree(name, clamp, B, monkeypatch):
    """H = 64: the DPP form against the LDS form (TRK_POINT3D_LDS64=1, read per call), bit-equal after 33 iterations, plain and via"""
    cm = handle(name, clamp)
    gp, w = OBJECTIVES[2]
    q0, qd0 = p3.walks(name, B, 64)
    for via in (None, (0.37, 5)):
        results = []
        for lds in ("0", "1"):
            monkeypatch.setenv("TRK_POINT3D_LDS64", lds)
            q, qd = dev(q0), dev(qd0)
            form = "lds" if lds == "1" else "dpp"                  # the switch is read per call, and each call says what it ran
            first = call(cm, q, qd, gp, w, via)
            assert ops.point3d_last_form() == form, (via, lds)
            plan = plan_of(cm, q, qd, gp, w, via, pin=5)
            plan.step(1)
            assert ops.point3d_last_form() == form, (via, lds)
            plan.step(32)
            assert ops.point3d_last_form() == form and plan.t == 33, (via, lds)
            results.append(list(first) + [q, qd, plan.m, plan.v, plan.cost])
        monkeypatch.delenv("TRK_POINT3D_LDS64")
        for x, y, what in zip(results[0], results[1], ("cost", "gq", "gqd", "q", "qd", "m", "v", "plan.cost")):
            assert torch.equal(x, y), (via, what, int((x != y).sum()))
        assert not torch.equal(results[0][3], dev(q0))
    # without the switch: DPP at horizon 64 only, LDS at every other horizon whatever the switch says
    for H, lds, form in ((64, None, "dpp"), (63, None, "lds"), (65, "0", "lds"), (128, "0", "lds"), (32, "1", "lds")):
        if lds is not None:
            monkeypatch.setenv("TRK_POINT3D_LDS64", lds)
        q, qd = (dev(x) for x in p3.walks(name, 2, H))
        call(cm, q, qd, gp, w, want_grad=False)
        assert ops.point3d_last_form() == form, (H, lds)
        monkeypatch.delenv("TRK_POINT3D_LDS64", raising=False)


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clamp", [("spheres", True), ("grid", False)])
def test_pins(name, clamp):
    cm = handle(name, clamp)
    B, H = 5, 63
    q0, qd0 = p3.walks(name, B, H)
    x0 = np.concatenate([q0, qd0], -1)
    for pin in range(16):
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(cm, q, qd, OBJECTIVES[0][0], OBJECTIVES[0][1], (1.0, 5), pin=pin)
        assert plan.pin == pin
        plan.step(33)
        x = np.concatenate([host(q), host(qd)], -1)
        held = p3.pin_masks(pin, B, H)
        assert np.array_equal(x[held].view(np.uint32), x0[held].view(np.uint32)), pin
        assert not host(plan.m)[held].any() and not host(plan.v)[held].any(), pin
        if pin == 0:
            assert (x[:, 0, :3] != x0[:, 0, :3]).any(-1).all() and (x[:, H - 1, :3] != x0[:, H - 1, :3]).any(-1).all()


def test_no_ops():
    cm = handle("spheres", True)
    gp, w = OBJECTIVES[0]
    q0, qd0 = p3.walks("spheres", 5, 63)
    # lr = 0 evaluates: the cost is written, nothing else
    for via in (None, (1.0, 5)):
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(cm, q, qd, gp, w, via, lr=0.0)
        plan.m.fill_(0.25); plan.v.fill_(0.5); plan.cost.fill_(float("nan"))
        cost = plan.step(7)
        assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((plan.m == 0.25).all()) and bool((plan.v == 0.5).all())
        assert torch.equal(cost, call(cm, q, qd, gp, w, via, want_grad=False)[0]) and plan.t == 0
        # n = 0 iterations: the same
        plan = plan_of(cm, q, qd, gp, w, via)
        plan.cost.fill_(float("nan"))
        assert torch.equal(plan.step(0), cost) and plan.t == 0 and torch.equal(q, dev(q0)) and not plan.m.any()
    # an empty batch returns at once
    e = torch.empty(0, 63, 3, device=DEV)
    assert plan_of(cm, e, e.clone(), gp, w, (1.0, 5)).step(3).shape == (0, 63)
    c, gq, gqd = call(cm, e, e.clone(), gp, w, (1.0, 5))
    assert c.shape == (0, 63) and gq.shape == (0, 63, 3) and gqd.shape == (0, 63, 3)
    # both calls stop at 256 samples, by name
    big = torch.zeros(1, 257, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        plan_of(cm, big, big.clone(), gp, w)
    with pytest.raises(NotImplementedError, match="256"):
        call(cm, big, big.clone(), gp, w)
    # a cost model with more columns than the point, and a weight on a term a point does not have
    arm = ops.CostHandle(hp.panda_cost_spec(hp.gold("cost_spheres3d"), hp.gold("panda_robot")), DEV)
    q, qd = dev(q0), dev(qd0)
    with pytest.raises(NotImplementedError, match="exactly one point"):
        ops.point3d_traj_cost_grad(arm, (0.0, 1.0, 1.0, 0.0), q, qd, 0.08, 1.0)
    with pytest.raises(NotImplementedError, match="exactly one point"):
        ops.Point3DAdamPlan(arm, (0.0, 1.0, 1.0, 0.0), q, qd, 0.08, 1.0).step(1)
    tracked = p3.spec_of("spheres", True)
    tracked = ops.CostHandle(type(tracked)(**{**vars(tracked), "ee_link": 0}), DEV)         # the point as a tracked link
    for weights, served in (((0.0, 1.0, 1.0, 0.5), False), ((1.0, 1.0, 1.0, 0.0), True), ((0.0, 1.0, 1.0, 0.0), True)):
        if served:                          # w_self without self pairs is a weight on a term the cost model does not have
            assert torch.equal(ops.point3d_traj_cost_grad(tracked, weights, q, qd, 0.08, 1.0)[0], call(cm, q, qd, (0.08, 1.0, 1.0), (1.0, 1.0))[0])
            continue
        with pytest.raises(NotImplementedError, match="w_self / w_ee"):
            ops.point3d_traj_cost_grad(tracked, weights, q, qd, 0.08, 1.0)
        with pytest.raises(NotImplementedError, match="w_self / w_ee"):
            ops.Point3DAdamPlan(tracked, weights, q, qd, 0.08, 1.0).step(1)
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0))          # no refused call touched the trajectories


SENTINEL = 12345.5


def off_boundary(shape):
    """a view 4 bytes off a 16-byte boundary inside a buffer of sentinels -> (view, buffer, the view's slice of the buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), SENTINEL, **TA)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + n].view(shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view, buf, slice(1, 1 + n)


def sentinels_intact(buf, sl):
    return bool((buf[:sl.start] == SENTINEL).all() and (buf[sl.stop:] == SENTINEL).all())


# 8 (the buffers' edges) and 9 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(4, 64), (3, 65)])
@pytest.mark.parametrize("name,clamp", [("spheres", True), ("grid", False), ("posed", True)])
def test_a_non_finite_trajectory_stays_alone_and_the_edges_stay_intact(name, clamp, B, H):
    """every buffer is a view 4 bytes off a 16-byte boundary with sentinels either side; one trajectory of NaN among finite ones, with
    the via term: every other trajectory's rows are bit-equal to a run without it"""
    cm = handle(name, clamp)
    gp, w, via = OBJECTIVES[0][0], OBJECTIVES[0][1], _abi.TrajVia(1.0, 5, *(x.data_ptr() for x in ops.via_point_weights(5, DEV)))
    wts, prior = _abi.RolloutWeights(0.0, w[0], w[1], 0.0), _abi.GpPrior(*gp)
    q0, qd0 = p3.walks(name, B, H)
    bad = B // 2
    others = [b for b in range(B) if b != bad]
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for poison in (False, True):
        (q, qb, qs), (qd, qdb, qds) = off_boundary((B, H, 3)), off_boundary((B, H, 3))
        (cost, cb, cs), (gq, gb, gs), (gqd, gdb, gds) = off_boundary((B, H)), off_boundary((B, H, 3)), off_boundary((B, H, 3))
        (m, mb, ms), (v, vb, vs), (pc, pb, ps) = off_boundary((B, H, 6)), off_boundary((B, H, 6)), off_boundary((B, H))
        q.copy_(dev(q0)); qd.copy_(dev(qd0)); m.zero_(); v.zero_()
        if poison:
            q[bad] = float("nan")
        rc = _lib.lib().trk_point3d_traj_cost_grad(cm._h, C.byref(wts), C.byref(prior), C.byref(via), q.data_ptr(), qd.data_ptr(), B, H,
                                                   cost.data_ptr(), gq.data_ptr(), gqd.data_ptr(), stream)
        assert rc == _abi.TRK_OK
        first = [t.clone() for t in (cost, gq, gqd)]
        adam = _abi.TrajAdam(LR, 0, 1, 3)
        rc = _lib.lib().trk_point3d_traj_adam_steps(cm._h, C.byref(wts), C.byref(prior), C.byref(via), C.byref(adam), q.data_ptr(),
                                                    qd.data_ptr(), m.data_ptr(), v.data_ptr(), B, H, pc.data_ptr(), stream)
        assert rc == _abi.TRK_OK
        torch.cuda.synchronize()
        for buf, sl in ((qb, qs), (qdb, qds), (cb, cs), (gb, gs), (gdb, gds), (mb, ms), (vb, vs), (pb, ps)):
            assert sentinels_intact(buf, sl)
        results.append(first + [t.clone() for t in (q, qd, m, v, pc)])
    for clean, dirty, what in zip(results[0], results[1], ("cost", "gq", "gqd", "q", "qd", "m", "v", "plan.cost")):
        assert torch.equal(clean[others], dirty[others]), what
        assert bool(torch.isfinite(clean).all()), what
    assert bool(torch.isnan(results[1][0][bad]).any()) and not torch.equal(results[0][3], dev(q0))
    assert torch.equal(results[0][0], results[0][7])                    # the loop's cost is the evaluation's


# 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["EnvSpheres3D", "EnvTableShelf"])
def test_through_the_task_and_a_captured_graph(env_name):
    task = tra.PlanningTask(env=getattr(tra, env_name)(tensor_args=TA), robot=tra.RobotPointMass3D(tensor_args=TA), obstacle_cutoff_margin=0.03,
                            clamp_sdf=True, tensor_args=TA)
    lo, hi = (host(v).astype(np.float64) for v in task.env.limits)
    rng = np.random.default_rng(7)
    start = rng.uniform(lo, hi, (9, 1, 3))
    q0 = (start + np.concatenate([np.zeros((9, 1, 3)), np.cumsum(rng.standard_normal((9, 63, 3)) * 0.02, axis=1)], 1)).astype(np.float32)
    qd0 = (rng.standard_normal((9, 64, 3)) * 0.3).astype(np.float32)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    via_task = task.point_mass_3d_optimizer(qa, qda, 5.0 / 64, 1.0, w_obj=20.0, w_ws=5.0, lr=LR, w_via=0.2, num_interpolation=5, pin_goal_vel=True)
    _, cm = task._fused_handles(DEV)
    direct = ops.Point3DAdamPlan(cm, (0.0, 20.0, 5.0, 0.0), qb, qdb, 5.0 / 64, 1.0, 1.0, LR, pin_goal_vel=True, w_via=0.2, num_interpolation=5)
    assert via_task.pin == 11 and via_task._via is not None and via_task.cm is cm
    for n in (1, 40):
        assert torch.equal(via_task.step(n), direct.step(n))
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(via_task.m, direct.m) and torch.equal(via_task.v, direct.v)
    assert via_task.t == 41 and not torch.equal(qa, dev(q0))
    # one replay of a captured 33-iteration call (two launches, the bias terms of its iterations by value) equals the eager call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        via_task.step(33)
    assert torch.equal(qa, qb) and torch.equal(via_task.m, direct.m)          # a capture records, it does not run
    graph.replay()
    direct.step(33)
    torch.cuda.synchronize()
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(via_task.m, direct.m) and torch.equal(via_task.v, direct.v)
    assert torch.equal(via_task.cost, direct.cost)


def test_fused_example_lowers_the_hinge_cost():
    spec = importlib.util.spec_from_file_location("plan_point_mass_3d", Path(hp.ROOT) / "examples" / "plan_point_mass_3d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after = mod.main(batch=128, horizon=64, iters=100, verbose=False, fused=True, via_cost=0)
    cost = dict(mod.LAST)
    print(f"fused example, 128 x 64, 100 iterations: free fraction {before:.3f} -> {after:.3f}, summed clamped hinge cost "
          f"{cost['cost_before']:.4g} -> {cost['cost_after']:.4g}")
    assert cost["cost_after"] < cost["cost_before"]
    assert after >= before

"""The arm's planning loop on the chip (trk_rollout_gp_adam_steps, generated kernel k_traj_adam; ops.ArmAdamPlan,
PlanningTask.rollout_adam_plan) on the Panda: evaluation and gradient against RolloutGpPlan and the fp64 oracle (oracle.rollout +
oracle.gp_prior), the Adam update against its formula in fp64 on the kernel's own moments, the grouping of iterations into launches
and calls to bit equality, the pin masks, the no-ops and refusals, the task's plan, a run-time compiled iiwa7 unit and the example.
Bounds: planar_traj_helpers (cost: rel 1e-5 on each half, summed; Adam: half an ulp + 2 x 6 x 2^-24 |update|), helpers (gradient:
DESIGN section 2's rel 1e-4 and per-element bound; kink_rows_ok for rows at a kink)."""
import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import planar_traj_helpers as pt
from helpers import rel_err
from torch_robotics_amd import codegen, jit, ops
from torch_robotics_amd.costmodel import CostModelSpec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
SHAPES = [(1, 64), (3, 64), (5, 64), (9, 32), (8, 8), (7, 2), (130, 1)]
SCENES = ["spheres", "shelf"]
CASES = [(s, c, "identity") for s in SCENES for c in (False, True)] + [("spheres", True, "moved")]
W = (1.0, 1.0, 1.0, 0.0)
DT, SIGMA, GPW, LR = 0.08, 1.0, 1.0, 1e-2
TOL_COST = 1e-5
_cache = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def setup(scene, clamp, base):
    """(kin, spec, ModelHandle, CostHandle, Oracle) of RobotPanda in a bundled scene, as PlanningTask builds the cost model"""
    key = (scene, clamp, base)
    if key not in _cache:
        from oracle.oracle import Oracle
        env = (tra.EnvSpheres3D if scene == "spheres" else tra.EnvTableShelf)(tensor_args=TA)
        task = tra.PlanningTask(env=env, robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05, clamp_sdf=clamp, tensor_args=TA)
        spec = task.build_cost_spec()
        kin = hp.model("panda_arm_no_gripper")
        if hp.ROLLOUT_BASES[base] is not None:
            kin.set_base_pose(hp.ROLLOUT_BASES[base])
        h, cm = ops.ModelHandle(kin), ops.CostHandle(spec, DEV)
        h.set_base_pose(kin.base_R, kin.base_t)
        _cache[key] = (kin, spec, h, cm, Oracle(kin, spec), task)
    return _cache[key]


def walks(kin, B, H, seed):
    """seeded random walks between random configurations; start and goal are drawn 15 % beyond the joint limits on either side, so some
    rows lie outside them"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(kin.lower_dof, np.float64), np.asarray(kin.upper_dof, np.float64)
    span = hi - lo
    a, b = (rng.uniform(lo - 0.15 * span, hi + 0.15 * span, (B, 1, len(lo))) for _ in range(2))
    s = np.linspace(0.0, 1.0, H).reshape(1, H, 1) if H > 1 else np.zeros((1, 1, 1))
    q = a + s * (b - a) + np.cumsum(rng.standard_normal((B, H, len(lo))) * 0.02, axis=1)
    return q.astype(np.float32), (rng.standard_normal((B, H, len(lo))) * 0.3).astype(np.float32)


def dof_limits(kin):
    lo, hi = np.zeros(kin.n_dofs), np.zeros(kin.n_dofs)
    for i in range(1, kin.n_links):
        d = int(kin.dof_idx[i])
        if d >= 0:
            lo[d], hi[d] = (kin.lower[i], kin.upper[i]) if kin.clamp[i] else (-np.pi, np.pi)
    return lo, hi


def inputs(kin, B, H, seed=None):
    """the walks of a shape, drawn once per robot (seed: another draw than the shape's own 1000 B + H)"""
    if not hasattr(kin, "lower_dof"):
        kin.lower_dof, kin.upper_dof = dof_limits(kin)
    key = ("in", kin.name, B, H, seed)
    if key not in _cache:
        _cache[key] = walks(kin, B, H, seed=1000 * B + H if seed is None else seed)
    return _cache[key]


def reference(o, oracle_lib, q, qd, w=W, dt=DT, sigma=SIGMA, gpw=GPW):
    B, H, D = q.shape
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    _, rc, rg = o.rollout(q64.reshape(-1, D), w, "f64")
    pf = oracle_lib.gp_factor_cost(q64, qd64, dt, sigma, gpw, "f64")
    _, pgq, pgqd = oracle_lib.gp_prior(q64, qd64, dt, sigma, gpw, "f64")
    return dict(hinge=rc.reshape(B, H), prior=pf, cost=rc.reshape(B, H) + pf, gc=rg.reshape(B, H, D), gq=rg.reshape(B, H, D) + pgq, gqd=pgqd)


def cost_bound(ref):
    return TOL_COST * np.abs(ref["hinge"]).max() + TOL_COST * np.abs(ref["prior"]).max()


def plan_of(h, cm, q, qd, lr=LR, pin=3, w=W, gpw=GPW, dt=DT, sigma=SIGMA):
    return ops.ArmAdamPlan(h, cm, w, q, qd, dt, sigma, gpw, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                           pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8))


def pin_masks(pin, B, H, D):
    m = np.zeros((B, H, 2 * D), bool)
    if pin & 1: m[:, 0, :D] = True
    if pin & 2: m[:, H - 1, :D] = True
    if pin & 4: m[:, 0, D:] = True
    if pin & 8: m[:, H - 1, D:] = True
    return m


def check_gradient(o, oracle_lib, got_q, got_qd, ref, q, qd, what, w=W, rows=None):
    """DESIGN section 2's gradient tolerance (rel 1e-4 and the per-element bound, helpers.grad_close) on gq and on gqd; for gq, whose
    collision half has kinks, on every ordinary row, with kink_rows_ok (its own cap of 3 rows) for the rest; at least half the batch
    ordinary.  The prior is smooth: gqd has no kinks, and at H = 1 there is no factor -- it is exactly zero.  w: the weights `ref` was
    formed with; rows: boolean (B H,), the samples whose gq is judged (default: all).  Returns the number of rows at a kink."""
    B, H, D = q.shape
    keep = np.ones(B * H, bool) if rows is None else np.asarray(rows, bool).reshape(B * H)
    n = int(keep.sum())
    g, r = got_q.reshape(B * H, D).astype(np.float64)[keep], ref["gq"].reshape(B * H, D)[keep]
    q = q.reshape(B * H, D)[keep]
    bound = hp.GRAD_RTOL * np.abs(r) + hp.GRAD_ATOL * max(1e-30, np.abs(r).max())
    bad = (np.abs(g - r) > bound).any(-1)
    print(f"{what}: {int(bad.sum())} of {n} rows at a kink; rel err of the rest {rel_err(g[~bad], r[~bad]) if (~bad).any() else 0.0:.2e}; "
          f"gqd excess {hp.grad_excess(got_qd, ref['gqd']) if H > 1 else 0.0:.3f}")
    assert 2 * int((~bad).sum()) >= n, what
    assert hp.grad_close(g[~bad], r[~bad], 1e-4, np.abs(r).max() / max(1e-30, np.abs(r[~bad]).max())), what
    prior_q = (ref["gq"] - ref["gc"]).reshape(B * H, D)[keep]
    assert hp.kink_rows_ok(g, r, q.reshape(n, D), lambda qp: o.rollout(qp, w, "f64")[2] + prior_q[rows_of(qp, q.reshape(n, D))], bad), what
    if H > 1:
        assert hp.grad_close(got_qd, ref["gqd"], 1e-4), what
    else:
        assert not np.asarray(got_qd).any(), what
    return int(bad.sum())


def rows_of(qp, q):
    """index of the sample each probe belongs to (probes lie within 3e-6 of their sample)"""
    return np.array([int(np.argmin(np.abs(q - p[None]).max(-1))) for p in qp])


# 1 + 2 + 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp,base", CASES)
def test_evaluation_gradient_and_update(scene, clamp, base, oracle_lib):
    kin, spec, h, cm, o, _ = setup(scene, clamp, base)
    D = kin.n_dofs
    for B, H in SHAPES:
        q0, qd0 = inputs(kin, B, H)
        ref = reference(o, oracle_lib, q0, qd0)
        q, qd = dev(q0), dev(qd0)
        # evaluation: lr = 0 writes nothing but cost
        ev = plan_of(h, cm, q, qd, lr=0.0)
        ev.m.fill_(7.0); ev.v.fill_(7.0)
        cost = host(ev.step(1)).copy()
        assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((ev.m == 7.0).all()) and bool((ev.v == 7.0).all()) and ev.t == 0
        gp = ops.RolloutGpPlan(h, cm, W, q, qd, DT, SIGMA, GPW, want_pos=False)
        gp.launch()
        torch.cuda.synchronize()
        err_gp, err64, bound = np.abs(cost - host(gp.cost)).max(), np.abs(cost - ref["cost"]).max(), cost_bound(ref)
        print(f"{scene} clamp={clamp} {base} {B}x{H}: cost vs RolloutGpPlan {err_gp:.3e}, vs fp64 {err64:.3e}, bound {bound:.3e}")
        assert err_gp <= bound and err64 <= bound, (B, H)
        # gradient: after one step from m = v = 0, m1 / 0.1f is the kernel's gradient up to two roundings
        plan = plan_of(h, cm, q, qd, pin=0)
        plan.step(1)
        m1, v1 = host(plan.m).copy(), host(plan.v).copy()
        g = m1.astype(np.float64) / float(np.float32(0.1))
        check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref, q0, qd0, f"{scene} clamp={clamp} {base} {B}x{H} vs fp64")
        ref_gp = dict(ref, gq=host(gp.gq).astype(np.float64), gqd=host(gp.gqd).astype(np.float64))
        check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref_gp, q0, qd0, f"{scene} clamp={clamp} {base} {B}x{H} vs RolloutGpPlan")
        # update: the first and the second step -- the moments against a validated gradient (step 1: the one just checked; step 2:
        # RolloutGpPlan's at the state after step 1), the new values against the formula in fp64 on the kernel's own moments
        x0 = np.concatenate([q0, qd0], -1)
        x1 = np.concatenate([host(q), host(qd)], -1)
        check_update(1, x0, np.zeros_like(m1), np.zeros_like(v1), g, x1, m1, v1)
        gp.launch()                                                      # reads q, qd in place: the gradient at x1
        g1 = np.concatenate([host(gp.gq), host(gp.gqd)], -1).astype(np.float64)
        plan.step(1)
        x2 = np.concatenate([host(q), host(qd)], -1)
        check_update(2, x1, m1, v1, g1, x2, host(plan.m), host(plan.v))


def check_update(step, x0, m0, v0, g, x1, m1, v1, lr=LR):
    """test_gpu_planar_traj.check_adam_step for 2 D components: m1 = 0.9 m0 + 0.1 g and v1 = 0.999 v0 + 0.001 g^2 within what the
    gradient tolerance d = 1e-4 |g| + 5e-6 max|g| allows (0.1 d; 0.001 (2 |g| d + d^2)) plus the roundings of the fma and the product,
    then the update formula on the returned moments"""
    x0, m0, v0, g, x1, m1, v1 = (np.asarray(t, np.float64) for t in (x0, m0, v0, g, x1, m1, v1))
    d = hp.GRAD_RTOL * np.abs(g) + hp.GRAD_ATOL * max(1e-30, np.abs(g).max())
    em = np.abs(m1 - (0.9 * m0 + 0.1 * g)) / (0.1 * d + 2.0 ** -22 * np.abs(m1))
    ev = np.abs(v1 - (0.999 * v0 + 0.001 * g * g)) / (0.001 * (2.0 * np.abs(g) * d + d * d) + 2.0 ** -22 * np.abs(v1) + 1e-300)
    bc1, rs = ops.planar_adam_bias_terms(step)
    upd = (float(np.float32(lr)) / bc1) * m1 / (np.sqrt(v1) * rs + 1e-8)
    bound = 0.5 * np.spacing(np.abs(x1).astype(np.float32)).astype(np.float64) + 2.0 * pt.ADAM_ROUNDINGS * 2.0 ** -24 * np.abs(upd)
    err = np.abs(x1 - (x0 - upd))
    print(f"adam step {step}: worst m / v recurrence error / bound {float(em.max()):.3f} / {float(ev.max()):.3f}, "
          f"worst update error / bound {float((err / bound).max()):.3f}")
    assert (em <= 1.0).all() and (ev <= 1.0).all()
    assert (err <= bound).all()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,clamp,base", [CASES[1], CASES[3], CASES[4]])
def test_grouping_of_iterations_is_bit_neutral(scene, clamp, base):
    kin, spec, h, cm, o, _ = setup(scene, clamp, base)
    for B, H in SHAPES:
        q0, qd0 = inputs(kin, B, H)
        for K in pt.GROUPINGS:
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            pa, pb = plan_of(h, cm, qa, qda), plan_of(h, cm, qb, qdb)
            ca = host(pa.step(K)).copy()
            cb = None
            for _ in range(K):
                c = pb.step(1)
                cb = host(c).copy() if cb is None else cb
            assert pa.t == pb.t == K
            assert np.array_equal(ca, cb), (B, H, K)
            for x, y in ((qa, qb), (qda, qdb), (pa.m, pb.m), (pa.v, pb.v)):
                assert torch.equal(x, y), (B, H, K)
            assert bool(torch.isfinite(qa).all()) and bool(torch.isfinite(pa.v).all())


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_all_pin_masks():
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    D = kin.n_dofs
    lo, hi = dof_limits(kin)
    for B, H in ((3, 64), (9, 32), (7, 2), (130, 1)):
        q0, qd0 = inputs(kin, B, H)
        outside = (q0 < lo) | (q0 > hi)
        assert outside.any()
        for pin in range(16):
            q, qd = dev(q0), dev(qd0)
            plan = plan_of(h, cm, q, qd, pin=pin)
            plan.step(3)
            pm = pin_masks(pin, B, H, D)
            x0, x1 = np.concatenate([q0, qd0], -1), np.concatenate([host(q), host(qd)], -1)
            assert np.array_equal(x1[pm], x0[pm]) and not host(plan.m)[pm].any() and not host(plan.v)[pm].any(), (B, H, pin)
            free = ~pm
            if H > 1 and free.any():              # (H = 2 with every pin set leaves nothing free)
                assert (host(plan.v)[free] > 0).mean() > 0.9, (B, H, pin)
        if H > 1:
            # outside the joint limits the collision gradient is zero (the clamp's mask), the prior still moves the component
            q, qd = dev(q0), dev(qd0)
            only = plan_of(h, cm, q, qd, pin=0, gpw=0.0)
            only.step(1)
            assert not host(only.m)[..., :D][outside].any(), (B, H)
            q, qd = dev(q0), dev(qd0)
            both = plan_of(h, cm, q, qd, pin=0)
            both.step(1)
            assert (host(q)[outside] != q0[outside]).mean() > 0.9 and host(both.m)[..., :D][outside].any(), (B, H)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_no_ops_and_refusals():
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    D = kin.n_dofs
    q0, qd0 = inputs(kin, 3, 64)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, cm, q, qd)
    plan.cost.fill_(-1.0)
    plan.step(0)                                                  # n_steps = 0: an evaluation
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and not plan.m.any() and not plan.v.any() and bool((plan.cost >= 0).all())
    e = torch.empty((0, 64, D), **TA)
    plan_of(h, cm, e, e.clone()).step(5)                          # batch = 0
    q1, qd1 = (dev(x) for x in inputs(kin, 130, 1))               # H = 1: no prior factor -- the velocities never move
    p1 = plan_of(h, cm, q1, qd1, pin=0)
    p1.step(2)
    assert torch.equal(qd1, dev(inputs(kin, 130, 1)[1])) and not p1.m[..., D:].any() and not torch.equal(q1, dev(inputs(kin, 130, 1)[0]))
    for H in (3, 48, 65, 128):
        t = torch.zeros((2, H, D), **TA)
        with pytest.raises(NotImplementedError, match="power of two"):
            plan_of(h, cm, t, t.clone())
    h2 = ops.ModelHandle(kin)
    h2.enable_specialized(False)
    with pytest.raises(NotImplementedError, match="switched off"):
        plan_of(h2, cm, q, qd).step(1)
    # a cost model no unit matches: another set of object-collision links
    spec2 = CostModelSpec(n_links_in=kin.n_links)
    spec2.obj_link_idx = np.asarray(spec.obj_link_idx, np.int32)[:-1]
    spec2.obj_link_margin = np.asarray(spec.obj_link_margin, np.float32)[:-1]
    spec2.objects = spec.objects
    spec2.ws_min, spec2.ws_max = spec.ws_min, spec.ws_max
    spec2.validate()
    with pytest.raises(NotImplementedError, match="bakes this cost model"):
        plan_of(h, ops.CostHandle(spec2, DEV), q, qd).step(1)
    assert torch.equal(q, dev(q0))


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_through_the_task():
    kin, spec, h, cm, o, task = setup("spheres", True, "identity")
    q0, qd0 = inputs(kin, 5, 64)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa = task.rollout_adam_plan(qa, qda, DT, SIGMA, gp_weight=GPW, w_self=W[0], w_obj=W[1], w_ws=W[2], lr=LR)
    pb = plan_of(h, cm, qb, qdb)
    ca, cb = pa.step(33), pb.step(33)
    assert torch.equal(ca, cb) and torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v)
    t = torch.zeros((2, 48, kin.n_dofs), **TA)
    with pytest.raises(NotImplementedError):
        task.rollout_adam_plan(t, t.clone(), DT, SIGMA)


def test_a_run_time_compiled_iiwa7_unit(oracle_lib):
    """iiwa7 with another collision template than its bundled unit's: the unit is compiled at run time by the same emitter"""
    from oracle.oracle import Oracle
    kin, tmpl = codegen.template_for("iiwa7")
    obj = list(tmpl.obj_links)[1:]
    env = tra.EnvSpheres3D(tensor_args=TA)
    spec = CostModelSpec(n_links_in=kin.n_links)
    spec.obj_link_idx = np.asarray(obj, np.int32)
    spec.obj_link_margin = np.linspace(0.08, 0.12, len(obj)).astype(np.float32)
    spec.objects = [ob.as_object() for ob in env.obj_fixed_list]
    spec.ws_min, spec.ws_max = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    spec.clamp_fields = 7
    spec.validate()
    assert not jit.has_matching_unit(kin, spec)
    jit.specialize_for_cost_spec(kin, spec)
    h, cm, o = ops.ModelHandle(kin), ops.CostHandle(spec, DEV), Oracle(kin, spec)
    B, H, D = 5, 64, kin.n_dofs
    q0, qd0 = inputs(kin, B, H)
    ref = reference(o, oracle_lib, q0, qd0)
    q, qd = dev(q0), dev(qd0)
    cost = host(plan_of(h, cm, q, qd, lr=0.0).step(1)).copy()
    assert np.abs(cost - ref["cost"]).max() <= cost_bound(ref)
    plan = plan_of(h, cm, q, qd, pin=0)
    plan.step(1)
    m1, v1 = host(plan.m).copy(), host(plan.v).copy()
    g = m1.astype(np.float64) / float(np.float32(0.1))
    check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref, q0, qd0, "iiwa7 (run-time unit)")
    check_update(1, np.concatenate([q0, qd0], -1), np.zeros_like(m1), np.zeros_like(v1), g, np.concatenate([host(q), host(qd)], -1), m1, v1)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_the_example_fused():
    import importlib.util
    path = hp.ROOT / "examples" / "plan_trajectories.py"
    sp = importlib.util.spec_from_file_location("plan_trajectories", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    stats = {}
    q, n_free, coll0 = mod.main(batch=64, horizon=64, iters=100, device="cuda:0", verbose=False, fused=True, stats=stats)
    print(f"example --fused: straight lines in collision {coll0:.2f}, free after {n_free}/64, collision cost {stats['cost_before']:.4f} -> {stats['cost_after']:.4f}")
    assert bool(torch.isfinite(q).all())
    assert n_free > round((1.0 - coll0) * 64)
    assert stats["cost_after"] < stats["cost_before"]

"""The arm's planning loop on the chip (k_traj_adam_bi/bg<BOX>, trk_rollout_gp_adam_steps, ops.ArmAdamPlan) on the terms, scenes,
robots and iterations that tests/test_gpu_arm_traj.py leaves out.  Same judges: the fp64 oracle (Oracle.rollout + oracle.gp_factor_cost
/ oracle.gp_prior) and RolloutGpPlan as a second opinion; same bounds: cost 1e-5 on each half on the batch's scale (cost_bound),
gradient DESIGN section 2 (check_gradient: helpers.grad_close, kink_rows_ok), update check_update.  The helpers are those of
tests/test_gpu_arm_traj.py, imported.

  the end-effector term, weights other than 0 and 1     test_ee_term_and_weights
  bg<true>: a moved base on a general scene             test_shelf_moved_base
  a voxel grid, alone and next to analytic spheres      test_grid_scenes, test_grid_and_spheres
    (bi<true> with a grid: no cooperative scoring)
  the bundled iiwa7 (D = 7) and UR10 (D = 6) units      test_bundled_units, test_ur10_pin_masks
  the prior's parameters (gp_a, gp_b, gp_c)             test_prior_parameters, test_prior_alone
  later iterations, `first_step + done + i`             test_later_iterations, test_grouped_launch_and_large_t
  horizons 4 and 16, writes past the end                the shapes (5, 16), (9, 4) throughout; test_nothing_written_outside
  a target changed under a live plan                    test_target_changed_under_a_live_plan, test_target_changed_through_the_task
  a tracked link the unit does not bake                 test_refusal_of_another_tracked_link

No bound of its own was needed.  The one candidate, the end-effector cost with ee_square = False (|e| instead of |e|^2), was measured
on the CPU with the oracle in fp32 against the oracle in fp64 on the inputs of test_ee_term_and_weights (every scene, setting, base,
weight and shape): the walks never bring the end effector within 0.19 m of the target, and the fp32 oracle's worst cost error is 0.077
of cost_bound with ee_square False and 0.077 with True, so the existing bound holds with a factor of 13 to spare for a kernel that
reorders fp32 operations and is used unchanged.  The prior's fp32 oracle stays below 0.11 of its half of the bound for the three
parameter sets of PRIORS.

The prior of the seeded walks is some hundred times the collision and end-effector terms, and cost_bound and the gradient's absolute
floor are on the batch's scale; so every case of sections 1 - 3 runs twice, with the prior as the issue sets it and with its weight 0
(GP_OFF), where the other terms are held to 1e-5 / 1e-4 of their own size.  (A factor 1.01 planted in the rotation adjoint of
k_traj_adam_bi passed ee_square = False with the prior on and failed with it off; w_ee left out of k_traj_adam_bg's rotation adjoint
failed both; one power of sigma too few in gp_a, gp_b, gp_c failed test_prior_parameters and test_prior_alone; tests/test_gpu_arm_traj.py
passed all three.)

Conditions on the inputs are asserted on the reference before any device work: the end-effector cost is positive on at least 90 % of
the samples; on a grid at least 95 % of the samples are judged (helpers.off_face_rows: fp32 kernel and fp64 oracle read the same cell)
and in each batch part of the arm is inside the grid's limits and part outside on at least 30 % of the samples each; every spec finds a
bundled unit (jit.has_matching_unit) -- nothing here compiles at run time."""
import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
from helpers import gold
from test_gpu_arm_traj import (DEV, DT, GPW, LR, SIGMA, TA, check_gradient, check_update, cost_bound, dev, dof_limits, host, inputs,
                               pin_masks, plan_of, reference, setup)
from torch_robotics_amd import codegen, jit, ops
from torch_robotics_amd.costmodel import CostModelSpec, make_object, sphere_prims

pytestmark = pytest.mark.gpu

CPU = dict(device="cpu", dtype=torch.float32)          # the environments are only read for their objects
GP0 = (DT, SIGMA, GPW)
# the walks' prior is some hundred times the collision and end-effector terms, and both bounds are on the batch's scale: every case of
# sections 1 - 3 runs a second time with the prior switched off, so that those terms are held to 1e-5 / 1e-4 of their own size
GP_OFF = (DT, SIGMA, 0.0)
BASES = ("identity", "moved")
EE_SETTINGS = {"square": {}, "plain": dict(ee_square=False), "rot_only": dict(ee_w_pos=0.0, ee_w_rot=2.5),
               "pos_only": dict(ee_w_pos=0.4, ee_w_rot=0.0)}
EE_WEIGHTS = [(1.0, 1.0, 1.0, 1.0), (0.3, 2.5, 0.7, 1.7), (0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 0.5)]
EE_SHAPES = [(3, 64), (5, 16), (9, 4), (7, 2)]
GRID_WEIGHTS = [(0.0, 1.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)]
GRID_SHAPES = [(3, 64), (9, 4)]
UNIT_WEIGHTS = [(1.0, 1.0, 1.0, 0.0), (0.3, 2.5, 0.7, 1.7)]
UNIT_SHAPES = [(3, 64), (5, 16), (130, 1)]
PRIORS = [(5.0 / 64, 0.5, 0.3), (0.02, 2.0, 1.0), (0.5, 0.25, 4.0)]
SENTINEL = 0x7FC0BEEF                                  # a quiet NaN's bit pattern
# the target of the bundled units' tracked link: a few decimetres from the base, turned about a tilted axis
UNIT_TARGET = np.eye(4, dtype=np.float32)
UNIT_TARGET[:3, :3] = hp.quat_rot64([0.8, 0.2, -0.4, 0.4]).astype(np.float32)
UNIT_TARGET[:3, 3] = [0.35, -0.2, 0.45]


# ---------------------------------------------------------------------------------------------------------------------------
# cost models
# ---------------------------------------------------------------------------------------------------------------------------
def panda_kin(base):
    kin = hp.model("panda_arm_no_gripper")
    if hp.ROLLOUT_BASES[base] is not None:
        kin.set_base_pose(hp.ROLLOUT_BASES[base])
    return kin


def panda_ee_spec(scene, ee_kw=None, clamp=False, target=None):
    """RobotPanda's cost model in a recorded scene with the recorded end-effector target (helpers.panda_cost_spec)"""
    g = gold("cost_spheres3d" if scene == "spheres" else "cost_table_shelf")
    spec = hp.panda_cost_spec(g, gold("panda_robot"), ee_target=gold("rollout_panda")["target"] if target is None else target, ee_kw=ee_kw)
    spec.clamp_fields = 7 if clamp else 0
    spec.validate()
    return spec


def rollout_grid(dims):
    return hp.address_grid(dims, hp.ROLLOUT_LO, hp.ROLLOUT_HI, seed=5)


def grid_spec(dims, spheres=False):
    extra = [make_object(sphere_prims(*hp.address_spheres(hp.ROLLOUT_LO, hp.ROLLOUT_HI)))] if spheres else []
    return hp.address_spec(rollout_grid(dims), extra_objects=extra, full=True)


def unit_case(ident, scene, clamp, base):
    """(KinModel, CostModelSpec) of a bundled unit's own collision template in a bundled scene"""
    kin, tmpl = codegen.template_for(ident)
    if hp.ROLLOUT_BASES[base] is not None:
        kin.set_base_pose(hp.ROLLOUT_BASES[base])
    env = (tra.EnvSpheres3D if scene == "spheres" else tra.EnvTableShelf)(tensor_args=CPU)
    obj = list(tmpl.obj_links)
    spec = CostModelSpec(n_links_in=kin.n_links)
    spec.obj_link_idx = np.asarray(obj, np.int32)
    spec.obj_link_margin = np.linspace(0.08, 0.12, len(obj)).astype(np.float32)
    spec.objects = [ob.as_object() for ob in env.obj_fixed_list]
    spec.ws_min, spec.ws_max = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    spec.ee_link, spec.ee_target = int(tmpl.ee_link), UNIT_TARGET.copy()
    spec.clamp_fields = 7 if clamp else 0
    spec.validate()
    return kin, spec


def handles(kin, spec):
    """(ModelHandle, CostHandle, Oracle); the spec must find a bundled unit: nothing is compiled at run time"""
    from oracle.oracle import Oracle
    assert jit.has_matching_unit(kin, spec)
    h, cm = ops.ModelHandle(kin), ops.CostHandle(spec, DEV)
    h.set_base_pose(kin.base_R, kin.base_t)
    return h, cm, Oracle(kin, spec)


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, on the reference alone
# ---------------------------------------------------------------------------------------------------------------------------
def ee_share(o, q0):
    """share of the samples whose end-effector cost is positive in fp64"""
    D = q0.shape[-1]
    return float((o.rollout(q0.reshape(-1, D).astype(np.float64), (0.0, 0.0, 0.0, 1.0), "f64")[1] > 0.0).mean())


def grid_rows(o, spec, q, strict=True):
    """the samples of q (..., D) that are judged on a grid (helpers.off_face_rows of the fp64 link positions); strict: the conditions
    of test_rollouts_on_a_non_cubic_grid on a batch -- 95 % judged, part of the arm inside the limits and part outside on 30 % each"""
    D = q.shape[-1]
    p64 = o.rollout(q.reshape(-1, D).astype(np.float64), (0.0, 1.0, 0.0, 0.0), "f64")[0]
    rows = hp.off_face_rows(p64, spec.grid)
    if strict:
        oli = np.asarray(spec.obj_link_idx)
        lo, hi = spec.grid["lim_min"].astype(np.float64), (spec.grid["lim_min"] + spec.grid["map_dim"]).astype(np.float64)
        outside = ((p64[:, oli] < lo) | (p64[:, oli] > hi)).any(-1)
        assert rows.mean() >= 0.95, float(rows.mean())
        assert outside.any(1).mean() >= 0.3 and (~outside).any(1).mean() >= 0.3, (float(outside.any(1).mean()), float((~outside).any(1).mean()))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the checks of test_gpu_arm_traj.test_evaluation_gradient_and_update on one shape
# ---------------------------------------------------------------------------------------------------------------------------
def cat(a, b):
    return np.concatenate([a, b], -1)


def evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, what, gp=GP0, lr=LR, grid_of=None, seed=None):
    """cost at lr = 0 against fp64 and RolloutGpPlan; the gradient from m1 / 0.1f against both; check_update at steps 1 and 2.  grid_of:
    the spec of a grid scene, whose costs and gradients are judged on the rows of grid_rows.  Returns (worst cost error / bound, rows
    at a kink against fp64)."""
    B, H = shape
    D = kin.n_dofs
    dt, sigma, gpw = gp
    q0, qd0 = inputs(kin, B, H, seed)
    ref = reference(o, oracle_lib, q0, qd0, w, dt, sigma, gpw)
    rows = np.ones(B * H, bool) if grid_of is None else grid_rows(o, grid_of, q0)
    q, qd = dev(q0), dev(qd0)
    kw = dict(w=w, gpw=gpw, dt=dt, sigma=sigma)
    ev = plan_of(h, cm, q, qd, lr=0.0, **kw)
    ev.m.fill_(7.0); ev.v.fill_(7.0)
    cost = host(ev.step(1)).copy()
    assert ops.last_dispatch() == "generated", what
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((ev.m == 7.0).all()) and bool((ev.v == 7.0).all()) and ev.t == 0
    gp_plan = ops.RolloutGpPlan(h, cm, w, q, qd, dt, sigma, gpw, want_pos=False)
    gp_plan.launch()
    torch.cuda.synchronize()
    r2 = rows.reshape(B, H)
    bound = cost_bound(dict(hinge=ref["hinge"][r2], prior=ref["prior"][r2]))
    err_gp, err64 = np.abs(cost - host(gp_plan.cost))[r2].max(), np.abs(cost - ref["cost"])[r2].max()
    print(f"{what} {B}x{H}: cost vs RolloutGpPlan {err_gp:.3e}, vs fp64 {err64:.3e}, bound {bound:.3e}, worst error / bound "
          f"{max(err_gp, err64) / bound:.3f}, judged {int(rows.sum())} of {B * H}")
    assert err_gp <= bound and err64 <= bound, (what, B, H)
    plan = plan_of(h, cm, q, qd, lr=lr, pin=0, **kw)
    plan.step(1)
    m1, v1 = host(plan.m).copy(), host(plan.v).copy()
    g = m1.astype(np.float64) / float(np.float32(0.1))
    kinks = check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref, q0, qd0, f"{what} {B}x{H} vs fp64", w=w, rows=rows)
    ref_gp = dict(ref, gq=host(gp_plan.gq).astype(np.float64), gqd=host(gp_plan.gqd).astype(np.float64))
    check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref_gp, q0, qd0, f"{what} {B}x{H} vs RolloutGpPlan", w=w, rows=rows)
    x0, x1 = cat(q0, qd0), cat(host(q), host(qd))
    check_update(1, x0, np.zeros_like(m1), np.zeros_like(v1), g, x1, m1, v1, lr=lr)
    gp_plan.launch()                                                 # reads q, qd in place: the gradient at x1
    g1 = cat(host(gp_plan.gq), host(gp_plan.gqd)).astype(np.float64)
    plan.step(1)
    x2 = cat(host(q), host(qd))
    # on a grid the two kernels are held to each other where the fp64 positions of x1 are off the cell faces, like every other gradient
    r1 = r2 if grid_of is None else grid_rows(o, grid_of, x1[..., :D], strict=False).reshape(B, H)
    check_update(2, x1[r1], m1[r1], v1[r1], g1[r1], x2[r1], host(plan.m)[r1], host(plan.v)[r1], lr=lr)
    return max(err_gp, err64) / bound, kinks


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("ee", list(EE_SETTINGS))
@pytest.mark.parametrize("scene", ["spheres", "shelf"])
def test_ee_term_and_weights(scene, ee, base, oracle_lib):
    """the `if (A.w.w_ee != 0.0f)` block of _emit_ee_terms -- rotation adjoints into the reverse pass, ee_w_pos, ee_w_rot, ee_square --
    under weights that are neither 0 nor 1, with every term switched off somewhere"""
    kin = panda_kin(base)
    spec = panda_ee_spec(scene, EE_SETTINGS[ee])
    h, cm, o = handles(kin, spec)
    worst = 0.0
    for shape in EE_SHAPES:
        q0, _ = inputs(kin, *shape)
        assert ee_share(o, q0) >= 0.9, shape                        # the term is never vacuous
        for w in EE_WEIGHTS:
            for gp in (GP0, GP_OFF):
                r, kinks = evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, f"{scene} ee={ee} {base} w={w} gpw={gp[2]:g}", gp=gp)
                worst = max(worst, r)
                if w == (0.0, 0.0, 0.0, 1.0) and EE_SETTINGS[ee].get("ee_square", True):
                    assert kinks == 0, (shape, w)                   # the squared term and the prior are smooth: every row is ordinary
    print(f"ee term {scene} {ee} {base}: worst cost error / bound {worst:.3f}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
def test_shelf_moved_base(clamp, oracle_lib):
    """k_traj_adam_bg<true>: a moved base on a scene with boxes"""
    kin = panda_kin("moved")
    h, cm, o = handles(kin, panda_ee_spec("shelf", clamp=clamp))
    for shape in EE_SHAPES:
        for w in ((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 1.0)):
            for gp in (GP0, GP_OFF):
                evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, f"shelf clamp={clamp} moved w={w} gpw={gp[2]:g}", gp=gp)


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("dims", hp.ROLLOUT_GRID_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_grid_scenes(dims, base, oracle_lib):
    """BOX = true for a voxel grid: bi<true> without the cooperative scoring of the constant link, bg<true>; part of the arm outside
    the grid's limits"""
    kin = panda_kin(base)
    spec = grid_spec(dims)
    h, cm, o = handles(kin, spec)
    for shape in GRID_SHAPES:
        for w in GRID_WEIGHTS:
            for gp in (GP0, GP_OFF):
                evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, f"grid {dims} {base} w={w} gpw={gp[2]:g}", gp=gp, grid_of=spec)


@pytest.mark.parametrize("base", BASES)
def test_grid_and_spheres(base, oracle_lib):
    """the minimum over a voxel grid and an analytic object"""
    kin = panda_kin(base)
    spec = grid_spec(hp.ROLLOUT_GRID_DIMS[0], spheres=True)
    assert len(spec.objects) == 2
    h, cm, o = handles(kin, spec)
    for shape in GRID_SHAPES:
        for w in GRID_WEIGHTS:
            for gp in (GP0, GP_OFF):
                evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, f"grid + spheres {base} w={w} gpw={gp[2]:g}", gp=gp, grid_of=spec)


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("scene", ["spheres", "shelf"])
@pytest.mark.parametrize("ident", ["iiwa7", "ur10"])
def test_bundled_units(ident, scene, clamp, base, oracle_lib):
    """the iiwa7 and UR10 kernels that every build compiles: D = 6 moves the [64][2D] transposes, the moment layout and every D + d"""
    kin, spec = unit_case(ident, scene, clamp, base)
    h, cm, o = handles(kin, spec)
    for shape in UNIT_SHAPES:
        assert ee_share(o, inputs(kin, *shape)[0]) >= 0.9, shape
        for w in UNIT_WEIGHTS:
            for gp in (GP0, GP_OFF):
                evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, w, shape, f"{ident} {scene} clamp={clamp} {base} w={w} gpw={gp[2]:g}", gp=gp)


def test_ur10_pin_masks():
    """test_gpu_arm_traj.test_all_pin_masks at D = 6"""
    kin, spec = unit_case("ur10", "spheres", True, "identity")
    h, cm, _ = handles(kin, spec)
    B, H, D = 3, 64, kin.n_dofs
    assert D == 6
    q0, qd0 = inputs(kin, B, H)
    x0 = cat(q0, qd0)
    for pin in range(16):
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, cm, q, qd, pin=pin, w=UNIT_WEIGHTS[1])
        plan.step(3)
        pm = pin_masks(pin, B, H, D)
        x1 = cat(host(q), host(qd))
        assert np.array_equal(x1[pm], x0[pm]) and not host(plan.m)[pm].any() and not host(plan.v)[pm].any(), pin
        assert (host(plan.v)[~pm] > 0).mean() > 0.9 and (x1[~pm] != x0[~pm]).mean() > 0.9, pin
        assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(qd).all())


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp", PRIORS, ids=lambda g: "-".join(f"{v:g}" for v in g))
def test_prior_parameters(gp, oracle_lib):
    """gp_a = 12 / (sigma^2 dt^3), gp_b = -6 / (sigma^2 dt^2), gp_c = 4 / (sigma^2 dt) over several orders of magnitude"""
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    for shape in ((3, 64), (9, 4)):
        evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, (1.0, 1.0, 1.0, 0.0), shape, f"prior {gp}", gp=gp)


@pytest.mark.parametrize("gp", PRIORS, ids=lambda g: "-".join(f"{v:g}" for v in g))
def test_prior_alone(gp, oracle_lib):
    """W = 0: no kinks, so every row is held to grad_close; the clamp's mask belongs to the collision half -- a position outside the
    joint limits still moves"""
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    lo, hi = dof_limits(kin)
    D = kin.n_dofs
    for shape in ((3, 64), (9, 4)):
        _, kinks = evaluation_gradient_and_update(kin, h, cm, o, oracle_lib, (0.0, 0.0, 0.0, 0.0), shape, f"prior alone {gp}", gp=gp)
        assert kinks == 0, shape
        q0, qd0 = inputs(kin, *shape)
        outside = (q0 < lo) | (q0 > hi)
        assert outside.any()
        q, qd = dev(q0), dev(qd0)
        plan = plan_of(h, cm, q, qd, pin=0, w=(0.0, 0.0, 0.0, 0.0), gpw=gp[2], dt=gp[0], sigma=gp[1])
        plan.step(1)
        assert (host(q)[outside] != q0[outside]).all() and (host(plan.m)[..., :D][outside] != 0).all(), shape


# 5 ---------------------------------------------------------------------------------------------------------------------------
def next_step_against_formula(plan, gp_plan, q, qd, t):
    """one more iteration from the plan's state after t iterations: RolloutGpPlan's gradient at that state, then check_update(t + 1)"""
    assert plan.t == t
    x, m, v = cat(host(q), host(qd)), host(plan.m).copy(), host(plan.v).copy()
    gp_plan.launch()
    g = cat(host(gp_plan.gq), host(gp_plan.gqd)).astype(np.float64)
    plan.step(1)
    print(f"iteration {t + 1}:", end=" ")
    check_update(t + 1, x, m, v, g, cat(host(q), host(qd)), host(plan.m), host(plan.v))


@pytest.mark.parametrize("t", [2, 32, 33, 64])
def test_later_iterations(t):
    """iterations 3, 33, 34 and 65 -- the first of a second and of a third launch and the one after -- against the update formula"""
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    q0, qd0 = inputs(kin, 3, 64)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, cm, q, qd, pin=0)
    gp_plan = ops.RolloutGpPlan(h, cm, (1.0, 1.0, 1.0, 0.0), q, qd, DT, SIGMA, GPW, want_pos=False)
    plan.step(t)
    next_step_against_formula(plan, gp_plan, q, qd, t)


def test_grouped_launch_and_large_t():
    """one step(40) -- launches of 32 and 8 iterations -- equals 40 single steps bit for bit, and the iteration after it follows the
    formula with the bias terms of step 41; the bias terms of step 1000 (bc1 = 1 in fp32, rsqrt_bc2 about 1.257)"""
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    q0, qd0 = inputs(kin, 3, 64)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa, pb = plan_of(h, cm, qa, qda, pin=0), plan_of(h, cm, qb, qdb, pin=0)
    pa.step(40)
    for _ in range(40):
        pb.step(1)
    assert pa.t == pb.t == 40
    for x, y in ((qa, qb), (qda, qdb), (pa.m, pb.m), (pa.v, pb.v)):
        assert torch.equal(x, y)
    next_step_against_formula(pa, ops.RolloutGpPlan(h, cm, (1.0, 1.0, 1.0, 0.0), qa, qda, DT, SIGMA, GPW, want_pos=False), qa, qda, 40)
    bc1, rs = ops.planar_adam_bias_terms(1000)
    assert bc1 == 1.0 and abs(rs - 1.257) < 1e-3
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, cm, q, qd, pin=0)
    plan.step(3)
    assert bool(plan.m.any()) and bool(plan.v.any())
    plan.t = 999
    next_step_against_formula(plan, ops.RolloutGpPlan(h, cm, (1.0, 1.0, 1.0, 0.0), q, qd, DT, SIGMA, GPW, want_pos=False), q, qd, 999)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def guarded(a, pad):
    """(flat int32 view of a sentinel-filled buffer, the contiguous fp32 view of its middle holding `a`)"""
    n = a.size
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV)
    mid = buf.view(torch.float32)[pad:pad + n].view(a.shape)
    mid.copy_(dev(a))
    assert mid.is_contiguous() and mid.data_ptr() == buf.data_ptr() + 4 * pad
    return buf, mid


@pytest.mark.parametrize("pad", [256, 257])          # 257: the trajectories are not 16-byte aligned, every wavefront takes the dword path
def test_nothing_written_outside(pad):
    """ragged last wavefronts, every pin mask, lr = 0 and lr > 0: the floats either side of q and qd keep their bits"""
    kin, spec, h, cm, o, _ = setup("spheres", True, "identity")
    for B, H in ((7, 2), (130, 1), (9, 32), (5, 16)):
        q0, qd0 = inputs(kin, B, H)
        n = q0.size
        for pin in range(16):
            for lr in (0.0, LR):
                bq, q = guarded(q0, pad)
                bqd, qd = guarded(qd0, pad)
                plan = plan_of(h, cm, q, qd, lr=lr, pin=pin)
                cost = plan.step(3)
                for b in (bq, bqd):
                    assert bool((b[:pad] == SENTINEL).all()) and bool((b[pad + n:] == SENTINEL).all()), (B, H, pin, lr)
                assert not bool(torch.isnan(cost).any()) and bool(torch.isfinite(plan.m).all()) and bool(torch.isfinite(plan.v).all())
                assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(qd).all())
                if lr == 0.0:
                    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)), (B, H, pin)


def far_target():
    """the recorded target moved by 0.4 m and turned by 90 degrees about z"""
    T = gold("rollout_panda")["target"].astype(np.float32).reshape(4, 4).copy()
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    T[:3, :3] = Rz @ T[:3, :3]
    T[:3, 3] += np.float32([-0.3, 0.25, -0.1])
    return T


def test_target_changed_under_a_live_plan(oracle_lib):
    """TrajAdamArgs.C is copied from the cost model on every call: CostHandle.set_ee_target between two steps takes effect"""
    from oracle.oracle import Oracle
    kin = panda_kin("identity")
    spec = panda_ee_spec("spheres", clamp=True)
    h, cm, o_old = handles(kin, spec)
    T2 = far_target()
    o_new = Oracle(kin, panda_ee_spec("spheres", clamp=True, target=T2))
    w = (1.0, 1.0, 1.0, 1.0)
    B, H = 3, 64
    q0, qd0 = inputs(kin, B, H)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(h, cm, q, qd, w=w)
    c1 = host(plan.step(1)).copy()
    ref0 = reference(o_old, oracle_lib, q0, qd0, w)
    assert np.abs(c1 - ref0["cost"]).max() <= cost_bound(ref0)
    x1q, x1qd = host(q).copy(), host(qd).copy()
    cm.set_ee_target(T2)
    c2 = host(plan.step(1)).copy()
    old, new = reference(o_old, oracle_lib, x1q, x1qd, w), reference(o_new, oracle_lib, x1q, x1qd, w)
    bound = max(cost_bound(old), cost_bound(new))
    assert (np.abs(new["cost"] - old["cost"]) > 20.0 * bound).mean() > 0.9          # the two targets are far apart on the reference
    print(f"target changed: cost vs fp64 with the new target {np.abs(c2 - new['cost']).max():.3e}, bound {cost_bound(new):.3e}, "
          f"worst error / bound {np.abs(c2 - new['cost']).max() / cost_bound(new):.3f}")
    assert np.abs(c2 - new["cost"]).max() <= cost_bound(new)
    assert (np.abs(c2 - old["cost"]) > 10.0 * bound).mean() > 0.9


def test_target_changed_through_the_task():
    """PlanningTask.set_ee_target under a plan of rollout_adam_plan, bit-equal to the direct plan on a cost model of its own"""
    env = tra.EnvSpheres3D(tensor_args=TA)
    task = tra.PlanningTask(env=env, robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05, clamp_sdf=True, tensor_args=TA)
    T1, T2 = gold("rollout_panda")["target"].astype(np.float32).reshape(4, 4), far_target()
    task.set_ee_target(T1)
    kin = panda_kin("identity")
    spec = task.build_cost_spec()
    h, cm, _ = handles(kin, spec)
    q0, qd0 = inputs(kin, 5, 64)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa = task.rollout_adam_plan(qa, qda, DT, SIGMA, gp_weight=GPW, w_self=1.0, w_obj=1.0, w_ws=1.0, w_ee=1.0, lr=LR)
    pb = plan_of(h, cm, qb, qdb, w=(1.0, 1.0, 1.0, 1.0))
    ca, cb = pa.step(1).clone(), pb.step(1).clone()
    assert torch.equal(ca, cb)
    task.set_ee_target(T2)
    cm.set_ee_target(T2)
    ca2, cb2 = pa.step(1), pb.step(1)
    assert torch.equal(ca2, cb2) and torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v)


def test_refusal_of_another_tracked_link():
    """w_ee != 0 on a cost model whose tracked link no unit bakes is refused before any device work; w_ee = 0 is served.  A run-time
    unit that an earlier test of the session loaded for another tracked link of the Panda (tests/test_gpu_api.py: panda_link7) serves
    that link rightly, so the link is one that neither a bundled nor a loaded unit tracks."""
    kin = panda_kin("identity")
    spec = panda_ee_spec("spheres", clamp=True)
    free = [l for l in range(2, 10) if not jit.has_matching_unit(kin, panda_ee_spec("spheres", dict(ee_link=l), clamp=True))]
    assert free
    spec.ee_link = free[0]
    spec.validate()
    h, cm = ops.ModelHandle(kin), ops.CostHandle(spec, DEV)
    q0, qd0 = inputs(kin, 3, 64)
    q, qd = dev(q0), dev(qd0)
    with pytest.raises(NotImplementedError, match="bakes this cost model"):
        plan_of(h, cm, q, qd, w=(1.0, 1.0, 1.0, 1.0)).step(1)
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0))
    plan_of(h, cm, q, qd, w=(1.0, 1.0, 1.0, 0.0)).step(1)
    assert ops.last_dispatch() == "generated" and not torch.equal(q, dev(q0))

"""The planning loop of the attached-point models on the chip (trk_rollout_points_gp_adam_steps, generated kernels k_padam_bi /
k_padam_bg<FAST>; ops.PointsAdamPlan, PlanningTask.points_adam_plan): the Panda with the 45 link spheres, with the grasped box, with
both -- on EnvSpheres3D, on EnvTableShelf and (the grasped box) on a voxel grid.

References: the fp64 oracle (Oracle.rollout_points + oracle.gp_prior / gp_factor_cost) and, on the GPU, what the loop replaces
(PointsRolloutPlan + ops.gp_prior_cost_grad).  The checks and bounds are tests/test_gpu_arm_traj.py's, through its own helpers
(reference, cost_bound, check_gradient, check_update, pin_masks: cost rel 1e-5 on each half, summed; gradient DESIGN section 2's rel
1e-4 and per-element bound with kink_rows_ok for rows at a kink; Adam half an ulp + 2 x 6 x 2^-24 |update|) -- PointsOracle gives the
oracle of a point model the interface those helpers call.  ops.gp_prior_cost_grad returns the prior's cost per trajectory, not per
factor: against the GPU reference the cost is held per sample with the prior off and per trajectory with it on, each under the same
rule (1e-5 of the largest value of each half of what is compared).
The inputs' hinge shares are held on the oracle alone in tests/test_points_adam_cpu.py."""
import copy

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
import planar_traj_helpers as pt
from test_gpu_arm_traj import (DT, GPW, LR, SHAPES, SIGMA, TOL_COST, check_gradient, check_update, cost_bound, dev, host, inputs, pin_masks,
                               reference)
from torch_robotics_amd import jit, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
W = (1.0, 1.0, 1.0, 0.0)
MODELS = ("spheres", "grasp", "both")
ROBOTS = {
    "spheres": lambda: tra.RobotPanda(link_sphere_model="panda", tensor_args=TA),
    "grasp": lambda: tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
    "both": lambda: tra.RobotPanda(link_sphere_model="panda", grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
}
ENVS = {
    "spheres": lambda: tra.EnvSpheres3D(tensor_args=TA),
    "shelf": lambda: tra.EnvTableShelf(tensor_args=TA),
    # 21 cells per axis: no cell face through the coordinates the model holds constant (tests/test_gpu_points_collision.py)
    "grid": lambda: tra.EnvSpheres3D(tensor_args=TA, precompute_sdf_obj_fixed=True, sdf_cell_size=0.096),
}
CASES = [(m, s, c, "identity") for m in MODELS for s in ("spheres", "shelf") for c in (True, False)]
MOVED = [(m, "spheres", True, "moved") for m in MODELS]
SENTINEL = 0x7FC0BEEF                                  # a quiet NaN's bit pattern
_cases = {}


class PointsOracle:
    """the fp64 oracle of a point model under the interface of Oracle.rollout, which test_gpu_arm_traj's helpers call"""

    def __init__(self, orc, pl, po):
        self.orc, self.pl, self.po = orc, pl, po

    def rollout(self, q, w, prec="f64"):
        return self.orc.rollout_points(self.pl, self.po, q, w, prec)


def _host_spec(spec):
    """the spec with the voxel grid's tables as host arrays (the oracle reads them on the CPU)"""
    if getattr(spec, "grid", None) is None:
        return spec
    h = copy.copy(spec)
    h.grid = {k: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in spec.grid.items()}
    return h


class Case:
    """one model in one scene at one base pose: the task, handles of its own (the task's stay at the identity) and the oracle"""

    def __init__(self, model, scene, clamp, base, oracle_lib, ee_target=None):
        self.robot = ROBOTS[model]()
        self.task = tra.PlanningTask(env=ENVS[scene](), robot=self.robot, obstacle_cutoff_margin=0.05, clamp_sdf=clamp, tensor_args=TA)
        if ee_target is not None:
            self.task.set_ee_target(ee_target)
        self.spec = self.task.build_cost_spec()
        self.pl, self.po = self.robot.collision_point_set()
        self.kin = copy.deepcopy(self.robot.diff_panda._kin)
        if hp.ROLLOUT_BASES[base] is not None:
            self.kin.set_base_pose(hp.ROLLOUT_BASES[base])
        self.h = ops.ModelHandle(self.kin)
        self.h.set_base_pose(self.kin.base_R, self.kin.base_t)
        self.ps, self.cm = ops.PointSetHandle(self.h, self.pl, self.po, DEV), ops.CostHandle(self.spec, DEV)
        assert self.ps.specialized
        self.oracle_lib = oracle_lib
        self.orc = oracle_lib.Oracle(self.kin, _host_spec(self.spec))
        self.o = PointsOracle(self.orc, self.pl, self.po)
        self.D = self.kin.n_dofs

    def rows(self, q):
        """the samples of q (..., D) that are judged: all, or on a voxel grid those whose tested points lie off the cell faces"""
        grid = getattr(self.orc.spec, "grid", None)
        n = int(np.prod(q.shape[:-1]))
        if grid is None:
            return np.ones(n, bool)
        pos64 = self.orc.fk_points(self.pl, self.po, q.reshape(-1, self.D).astype(np.float64), "f64")
        return hp.off_face_rows(pos64[:, [int(i) for i in self.spec.obj_link_idx]], grid)


def case_of(key, oracle_lib):
    if key not in _cases:
        _cases[key] = Case(*key, oracle_lib)
    return _cases[key]


def plan_of(c, q, qd, lr=LR, pin=3, w=W, gpw=GPW, dt=DT, sigma=SIGMA, ps=None, cm=None):
    return ops.PointsAdamPlan(ps or c.ps, cm or c.cm, w, q, qd, dt, sigma, gpw, lr, pin_start=bool(pin & 1), pin_goal=bool(pin & 2),
                              pin_start_vel=bool(pin & 4), pin_goal_vel=bool(pin & 8))


def cat(a, b):
    return np.concatenate([a, b], -1)


class GpuReference:
    """what the loop replaces: PointsRolloutPlan + ops.gp_prior_cost_grad, reading q, qd in place"""

    def __init__(self, c, q, qd, w, dt, sigma, gpw, ps=None, cm=None):
        self.plan = ops.PointsRolloutPlan(ps or c.ps, cm or c.cm, w, q, want_pos=False)
        self.q, self.qd, self.gp = q, qd, (dt, sigma, gpw)

    def launch(self):
        self.plan.launch()
        assert ops.last_dispatch() == "generated"
        dt, sigma, gpw = self.gp
        pc, pgq, pgqd = ops.gp_prior_cost_grad(self.q, self.qd, dt, sigma, gpw)
        torch.cuda.synchronize()
        self.hinge = host(self.plan.cost).astype(np.float64)
        self.prior_traj = host(pc).astype(np.float64)
        self.gq = host(self.plan.gq).astype(np.float64) + host(pgq).astype(np.float64)
        self.gqd = host(pgqd).astype(np.float64)


def evaluation_gradient_and_update(c, oracle_lib, w, shape, what, gpw=GPW, dt=DT, sigma=SIGMA, lr=LR, ps=None, cm=None, o=None, update=True):
    """assertions 1 - 3 on one shape: cost at lr = 0 against fp64 and the GPU reference; the gradient from m1 / 0.1f against both;
    check_update at steps 1 and 2"""
    B, H = shape
    D, o = c.D, o or c.o
    q0, qd0 = inputs(c.kin, B, H)
    ref = reference(o, oracle_lib, q0, qd0, w, dt, sigma, gpw)
    rows = c.rows(q0)
    r2 = rows.reshape(B, H)
    q, qd = dev(q0), dev(qd0)
    kw = dict(w=w, gpw=gpw, dt=dt, sigma=sigma, ps=ps, cm=cm)
    ev = plan_of(c, q, qd, lr=0.0, **kw)
    ev.m.fill_(7.0); ev.v.fill_(7.0)
    cost = host(ev.step(1)).copy()
    assert ops.last_dispatch() == "generated", what
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and bool((ev.m == 7.0).all()) and bool((ev.v == 7.0).all()) and ev.t == 0
    gr = GpuReference(c, q, qd, w, dt, sigma, gpw, ps, cm)
    gr.launch()
    bound = cost_bound(dict(hinge=ref["hinge"][r2], prior=ref["prior"][r2]))
    err64 = np.abs(cost - ref["cost"])[r2].max()
    # the GPU reference has the prior per trajectory: trajectories whose samples are all judged, 1e-5 of each half's largest sum
    full = r2.all(1)
    tsum = cost.astype(np.float64).sum(1)
    tbound = err_gpu = 0.0                                           # (a grid scene may leave no trajectory whole: costs_per_term holds the samples)
    if full.any():
        tbound = TOL_COST * np.abs(gr.hinge.sum(1)[full]).max() + TOL_COST * np.abs(gr.prior_traj[full]).max()
        err_gpu = np.abs(tsum - (gr.hinge.sum(1) + gr.prior_traj))[full].max()
    print(f"{what} {B}x{H}: cost vs fp64 {err64:.3e} (bound {bound:.3e}), per trajectory vs the GPU reference {err_gpu:.3e} (bound {tbound:.3e}), "
          f"judged {int(rows.sum())} of {B * H}")
    assert err64 <= bound and err_gpu <= tbound, (what, B, H)
    if not update:
        return
    plan = plan_of(c, q, qd, lr=lr, pin=0, **kw)
    plan.step(1)
    m1, v1 = host(plan.m).copy(), host(plan.v).copy()
    g = m1.astype(np.float64) / float(np.float32(0.1))
    check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref, q0, qd0, f"{what} {B}x{H} vs fp64", w=w, rows=rows)
    ref_gpu = dict(ref, gq=gr.gq, gqd=gr.gqd)
    check_gradient(o, oracle_lib, g[..., :D], g[..., D:], ref_gpu, q0, qd0, f"{what} {B}x{H} vs PointsRolloutPlan + gp_prior", w=w, rows=rows)
    x0, x1 = cat(q0, qd0), cat(host(q), host(qd))
    check_update(1, x0, np.zeros_like(m1), np.zeros_like(v1), g, x1, m1, v1, lr=lr)
    gr.launch()                                                      # reads q, qd in place: the gradient at x1
    g1 = cat(gr.gq, gr.gqd)
    plan.step(1)
    x2 = cat(host(q), host(qd))
    r1 = c.rows(x1[..., :D]).reshape(B, H)
    check_update(2, x1[r1], m1[r1], v1[r1], g1[r1], x2[r1], host(plan.m)[r1], host(plan.v)[r1], lr=lr)


def costs_per_term(c, oracle_lib, shape, what, weights):
    """assertion 1 with the prior off and with each weight off in turn: the cost alone, per sample against fp64 and against
    PointsRolloutPlan (the prior off: the kernel's cost is the rollout's)"""
    B, H = shape
    q0, qd0 = inputs(c.kin, B, H)
    q, qd = dev(q0), dev(qd0)
    r2 = c.rows(q0).reshape(B, H)
    for w, gpw in weights:
        ref = reference(c.o, oracle_lib, q0, qd0, w, DT, SIGMA, gpw)
        cost = host(plan_of(c, q, qd, lr=0.0, w=w, gpw=gpw).step(1)).copy()
        bound = cost_bound(dict(hinge=ref["hinge"][r2], prior=ref["prior"][r2]))
        err64 = np.abs(cost - ref["cost"])[r2].max()
        msg = f"{what} {B}x{H} w={w} gpw={gpw:g}: cost vs fp64 {err64:.3e} (bound {bound:.3e})"
        assert err64 <= bound, msg
        if gpw == 0.0:
            roll = ops.PointsRolloutPlan(c.ps, c.cm, w, q, want_pos=False)
            roll.launch()
            err_gpu = np.abs(cost - host(roll.cost))[r2].max()
            msg += f", vs PointsRolloutPlan {err_gpu:.3e}"
            assert err_gpu <= bound, msg
        print(msg)


TERMS_OFF = [(W, 0.0), ((0.0, 1.0, 1.0, 0.0), GPW), ((1.0, 0.0, 1.0, 0.0), GPW), ((1.0, 1.0, 0.0, 0.0), GPW)]


# 1 + 2 + 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,scene,clamp,base", CASES + MOVED)
def test_evaluation_gradient_and_update(model, scene, clamp, base, oracle_lib):
    c = case_of((model, scene, clamp, base), oracle_lib)
    what = f"{model} {scene} clamp={clamp} {base}"
    for shape in SHAPES:
        evaluation_gradient_and_update(c, oracle_lib, W, shape, what)
        costs_per_term(c, oracle_lib, shape, what, TERMS_OFF)


def test_grasped_box_on_a_voxel_grid(oracle_lib):
    c = case_of(("grasp", "grid", True, "identity"), oracle_lib)
    assert getattr(c.orc.spec, "grid", None) is not None
    for shape in SHAPES:
        q0, _ = inputs(c.kin, *shape)
        assert c.rows(q0).mean() >= 0.9
        evaluation_gradient_and_update(c, oracle_lib, W, shape, "grasp on a voxel grid")
        costs_per_term(c, oracle_lib, shape, "grasp on a voxel grid", TERMS_OFF[:1])


def far_target():
    """the recorded target moved by 0.4 m and turned by 90 degrees about z"""
    T = hp.gold("rollout_panda")["target"].astype(np.float32).reshape(4, 4).copy()
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    T[:3, :3] = Rz @ T[:3, :3]
    T[:3, 3] += np.float32([-0.3, 0.25, -0.1])
    return T


def test_ee_term_and_a_target_changed_under_a_live_plan(oracle_lib):
    """w_ee = 1 (the `if (A.w.w_ee != 0.0f)` block of _points_ee_term), then CostHandle.set_ee_target between two steps: TrajAdamArgs.C
    is copied from the cost model on every call"""
    T1, T2 = hp.gold("rollout_panda")["target"].astype(np.float32).reshape(4, 4), far_target()
    c = Case("grasp", "spheres", True, "identity", oracle_lib, ee_target=T1)
    w = (1.0, 1.0, 1.0, 1.0)
    share = float((c.o.rollout(inputs(c.kin, 5, 64)[0].reshape(-1, c.D).astype(np.float64), (0.0, 0.0, 0.0, 1.0), "f64")[1] > 0.0).mean())
    assert share > 0.9, share
    for shape in SHAPES:
        evaluation_gradient_and_update(c, oracle_lib, w, shape, "grasp w_ee=1")
        costs_per_term(c, oracle_lib, shape, "grasp w_ee=1", [(w, 0.0), ((0.0, 0.0, 0.0, 1.0), 0.0), ((1.0, 1.0, 1.0, 0.0), GPW)])
    spec2 = copy.copy(c.spec)
    spec2.ee_target = T2
    o_new = PointsOracle(oracle_lib.Oracle(c.kin, spec2), c.pl, c.po)
    B, H = 3, 64
    q0, qd0 = inputs(c.kin, B, H)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(c, q, qd, w=w)
    c1 = host(plan.step(1)).copy()
    ref0 = reference(c.o, oracle_lib, q0, qd0, w)
    assert np.abs(c1 - ref0["cost"]).max() <= cost_bound(ref0)
    x1q, x1qd = host(q).copy(), host(qd).copy()
    c.cm.set_ee_target(T2)
    c2 = host(plan.step(1)).copy()
    old, new = reference(c.o, oracle_lib, x1q, x1qd, w), reference(o_new, oracle_lib, x1q, x1qd, w)
    bound = max(cost_bound(old), cost_bound(new))
    assert (np.abs(new["cost"] - old["cost"]) > 20.0 * bound).mean() > 0.9          # the two targets are far apart on the reference
    assert np.abs(c2 - new["cost"]).max() <= cost_bound(new)
    assert (np.abs(c2 - old["cost"]) > 10.0 * bound).mean() > 0.9


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,scene,clamp,base", [("spheres", "spheres", True, "identity"), ("grasp", "shelf", False, "identity"),
                                                    ("both", "spheres", True, "moved")])
def test_grouping_of_iterations_is_bit_neutral(model, scene, clamp, base, oracle_lib):
    c = case_of((model, scene, clamp, base), oracle_lib)
    for B, H in SHAPES:
        q0, qd0 = inputs(c.kin, B, H)
        for K in pt.GROUPINGS:
            qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
            pa, pb = plan_of(c, qa, qda), plan_of(c, qb, qdb)
            ca = host(pa.step(K)).copy()
            cb = None
            for _ in range(K):
                cc = pb.step(1)
                cb = host(cc).copy() if cb is None else cb
            assert pa.t == pb.t == K
            assert np.array_equal(ca, cb), (B, H, K)
            for x, y in ((qa, qb), (qda, qdb), (pa.m, pb.m), (pa.v, pb.v)):
                assert torch.equal(x, y), (B, H, K)
            assert bool(torch.isfinite(qa).all()) and bool(torch.isfinite(pa.v).all())


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_all_pin_masks(model, oracle_lib):
    c = case_of((model, "spheres", True, "identity"), oracle_lib)
    D = c.D
    for B, H in ((3, 64), (9, 32), (7, 2), (130, 1)):
        q0, qd0 = inputs(c.kin, B, H)
        for pin in range(16):
            q, qd = dev(q0), dev(qd0)
            plan = plan_of(c, q, qd, pin=pin)
            plan.step(3)
            pm = pin_masks(pin, B, H, D)
            x0, x1 = cat(q0, qd0), cat(host(q), host(qd))
            assert np.array_equal(x1[pm], x0[pm]) and not host(plan.m)[pm].any() and not host(plan.v)[pm].any(), (B, H, pin)
            free = ~pm
            if H > 1 and free.any():              # (H = 2 with every pin set leaves nothing free)
                assert (host(plan.v)[free] > 0).mean() > 0.9, (B, H, pin)


# 6 + 10 ----------------------------------------------------------------------------------------------------------------------
def test_no_ops_and_refusals(oracle_lib):
    c = case_of(("grasp", "spheres", True, "identity"), oracle_lib)
    D = c.D
    q0, qd0 = inputs(c.kin, 3, 64)
    q, qd = dev(q0), dev(qd0)
    plan = plan_of(c, q, qd)
    plan.cost.fill_(-1.0)
    plan.step(0)                                                  # n_steps = 0: an evaluation
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and not plan.m.any() and not plan.v.any() and bool((plan.cost >= 0).all())
    e = torch.empty((0, 64, D), **TA)
    plan_of(c, e, e.clone()).step(5)                              # batch = 0
    q1, qd1 = (dev(x) for x in inputs(c.kin, 130, 1))             # H = 1: no prior factor -- the velocities never move
    p1 = plan_of(c, q1, qd1, pin=0)
    p1.step(2)
    assert torch.equal(qd1, dev(inputs(c.kin, 130, 1)[1])) and not p1.m[..., D:].any() and not torch.equal(q1, dev(inputs(c.kin, 130, 1)[0]))
    for H in (3, 48, 65, 128):
        t = torch.zeros((2, H, D), **TA)
        with pytest.raises(NotImplementedError, match="power of two"):
            plan_of(c, t, t.clone())
    with pytest.raises(ValueError, match="float32"):
        plan_of(c, q.half(), qd.half())
    for kw in (dict(w_via=0.2), dict(num_interpolation=5), dict(w_via=0.2, num_interpolation=5)):
        with pytest.raises(NotImplementedError, match="via-point term"):
            ops.PointsAdamPlan(c.ps, c.cm, W, q, qd, DT, SIGMA, **kw)
    # generated kernels switched off: there is no table-driven form
    h2 = ops.ModelHandle(c.kin)
    h2.enable_specialized(False)
    ps2 = ops.PointSetHandle(h2, c.pl, c.po, DEV)
    with pytest.raises(NotImplementedError, match="switched off"):
        plan_of(c, q, qd, ps=ps2).step(1)
    # a cost model whose column sets no unit bakes: one collision column fewer
    spec2 = copy.copy(c.spec)
    spec2.obj_link_idx = np.asarray(c.spec.obj_link_idx, np.int32)[:-1]
    spec2.obj_link_margin = np.asarray(c.spec.obj_link_margin, np.float32)[:-1]
    spec2.validate()
    with pytest.raises(NotImplementedError, match="bakes this cost model"):
        plan_of(c, q, qd, cm=ops.CostHandle(spec2, DEV)).step(1)
    # the point set of another model
    other = ops.ModelHandle(copy.deepcopy(c.kin))
    with pytest.raises(ValueError, match="does not belong to this model"):
        p = plan_of(c, q, qd)
        p._args = (other._h,) + p._args[1:]
        p.step(1)
    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0))


# 7 ---------------------------------------------------------------------------------------------------------------------------
def guarded(a, pad):
    """(flat int32 view of a sentinel-filled buffer, the contiguous fp32 view of its middle holding `a`)"""
    n = a.size
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV)
    mid = buf.view(torch.float32)[pad:pad + n].view(a.shape)
    mid.copy_(dev(a))
    assert mid.is_contiguous() and mid.data_ptr() == buf.data_ptr() + 4 * pad
    return buf, mid


@pytest.mark.parametrize("pad", [256, 257])          # 257: the rows are not 16-byte aligned, every wavefront takes the dword path
def test_nothing_written_outside(pad, oracle_lib):
    """ragged last wavefronts, lr = 0 and lr > 0: the floats either side of q, qd, m and v keep their bits"""
    c = case_of(("both", "spheres", True, "identity"), oracle_lib)
    D = c.D
    for B, H in ((7, 2), (130, 1), (9, 32), (5, 64)):
        q0, qd0 = inputs(c.kin, B, H)
        z = np.zeros((B, H, 2 * D), np.float32)
        for pin in (0, 3, 15):
            for lr in (0.0, LR):
                bufs = [guarded(a, pad) for a in (q0, qd0, z, z)]
                (bq, q), (bqd, qd), (bm, m), (bv, v) = bufs
                plan = plan_of(c, q, qd, lr=lr, pin=pin)
                plan.m, plan.v = m, v
                plan._bind()
                cost = plan.step(3)
                torch.cuda.synchronize()
                for (b, mid), a in zip(bufs, (q0, qd0, z, z)):
                    assert bool((b[:pad] == SENTINEL).all()) and bool((b[pad + a.size:] == SENTINEL).all()), (B, H, pin, lr)
                assert not bool(torch.isnan(cost).any()) and all(bool(torch.isfinite(t).all()) for t in (q, qd, m, v))
                if lr == 0.0:
                    assert torch.equal(q, dev(q0)) and torch.equal(qd, dev(qd0)) and not m.any() and not v.any(), (B, H, pin)
                elif pin == 0:                                   # (H = 2 with every pin set leaves nothing free)
                    assert bool(m.any()) and bool(v.any()), (B, H, pin)


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_through_the_task(model, oracle_lib):
    c = case_of((model, "spheres", True, "identity"), oracle_lib)
    q0, qd0 = inputs(c.kin, 5, 64)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa = c.task.points_adam_plan(qa, qda, DT, SIGMA, gp_weight=GPW, w_self=W[0], w_obj=W[1], w_ws=W[2], lr=LR)
    assert isinstance(pa, ops.PointsAdamPlan) and pa._fn.__name__ == "trk_rollout_points_gp_adam_steps"
    pb = plan_of(c, qb, qdb)
    ca, cb = pa.step(33), pb.step(33)
    assert torch.equal(ca, cb) and torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v)
    assert not torch.equal(qa, dev(q0))
    t = torch.zeros((2, 48, c.D), **TA)
    with pytest.raises(NotImplementedError, match="power of two"):
        c.task.points_adam_plan(t, t.clone(), DT, SIGMA)
    with pytest.raises(NotImplementedError, match="link-column"):
        c.task.rollout_adam_plan(qa, qda, DT, SIGMA)
    with pytest.raises(NotImplementedError, match="link-column"):
        c.task.rollout_gp_plan(qa, qda, DT, SIGMA)


def test_a_captured_graph_replays_the_loop(oracle_lib):
    """no host synchronisation inside the call: 33 iterations (two launches) captured once, replayed, equal the eager plan bit for bit"""
    c = case_of(("grasp", "spheres", True, "identity"), oracle_lib)
    q0, qd0 = inputs(c.kin, 5, 64)
    qa, qda, qb, qdb = dev(q0), dev(qd0), dev(q0), dev(qd0)
    pa, pb = plan_of(c, qa, qda), plan_of(c, qb, qdb)
    pa.step(0)                                                     # everything lazy is initialised before the capture
    pa._adam.first_step, pa._adam.n_steps = 1, 33
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pa._launch(None)
    assert torch.equal(qa, dev(q0))                                # captured, not run
    g.replay()
    pb.step(33)
    torch.cuda.synchronize()
    assert torch.equal(qa, qb) and torch.equal(qda, qdb) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v) and torch.equal(pa.cost, pb.cost)


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_run_time_unit_gets_the_planning_loop(oracle_lib):
    """A Panda holding a box of another size (the grasp golden's point set, stretched: no ahead-of-time unit) compiled at run time
    (jit.specialize_points): its planning-loop kernels are compiled when the first plan binds the entry, and meet assertions 1 - 3.
    (This test includes a hipcc compile of the unit on a cold cache.)"""
    assert jit.hipcc_available()           # (the hipRTC fall-back carries no planning-loop kernel)
    m, pl, po, spec = hp.grasp_panda_setup()
    po = (po * np.float32(1.25)).astype(np.float32)
    spec.clamp_fields = 7
    spec.validate()
    ident = jit.specialize_points(m, pl, po, spec)
    assert ident
    h = ops.ModelHandle(m)
    ps, cm = ops.PointSetHandle(h, pl, po, DEV), ops.CostHandle(spec, DEV)
    assert ps.specialized

    class RunTime:
        kin, D = m, m.n_dofs
        o = PointsOracle(oracle_lib.Oracle(m, spec), pl, po)
        rows = staticmethod(lambda q: np.ones(int(np.prod(q.shape[:-1])), bool))
    RunTime.ps, RunTime.cm = ps, cm
    for shape in ((5, 64), (9, 32), (130, 1)):
        evaluation_gradient_and_update(RunTime, oracle_lib, W, shape, "run-time unit (stretched grasped box)")
    assert (jit.JIT_DIR / f"spec_{ident}_padam.so").exists() and (ident, "padam") not in jit._pending
    assert jit.load_satellite_units(m, "padam") == []                   # idempotent


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_the_example_fused_with_a_grasped_box():
    import importlib.util
    path = hp.ROOT / "examples" / "plan_trajectories.py"
    sp = importlib.util.spec_from_file_location("plan_trajectories", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    stats = {}
    q, n_free, coll0 = mod.main(batch=64, horizon=64, iters=64, device="cuda:0", verbose=False, fused=True, stats=stats, model="grasp")
    print(f"example --model grasp --fused: straight lines in collision {coll0:.2f}, free after {n_free}/64, mean collision cost "
          f"{stats['cost_before']:.4f} -> {stats['cost_after']:.4f}")
    assert bool(torch.isfinite(q).all())
    assert stats["cost_after"] < stats["cost_before"]
    with pytest.raises(NotImplementedError, match="via-cost"):
        mod.main(batch=4, horizon=8, iters=1, device="cuda:0", verbose=False, fused=True, via_cost=5, model="grasp")


def test_the_example_eager_loop_of_a_point_model():
    """the eager route of --model spheres (rollout_plan + gp_prior_cost_grad + torch.optim.Adam) runs and lowers the collision cost"""
    import importlib.util
    path = hp.ROOT / "examples" / "plan_trajectories.py"
    sp = importlib.util.spec_from_file_location("plan_trajectories", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    q, n_free, coll0 = mod.main(batch=16, horizon=16, iters=8, device="cuda:0", verbose=False, model="spheres")
    assert bool(torch.isfinite(q).all()) and q.shape == (16, 16, 7)

#!/usr/bin/env python3
"""A small batch trajectory optimiser on the fused kernels -- how an external planner (the consumers of the reference's
`PlanningTask.get_collision_fields()` / `compute_collision_cost`) sits on this package.

B straight-line initial trajectories from a start configuration to B sampled collision-free goals are improved by Adam
on   w_obj * (self + object + workspace collision hinges)  +  (constant-velocity GP prior on q, qd)
where every cost / gradient evaluation is ONE launch of `trk_rollout_gp_cost_grad` over all (B x H) configurations (the fused rollout
with the GP prior fused in: `task.rollout_gp_plan`); the result is validated the way the reference does it after planning
(`get_trajs_collision_and_free`: 5 via points per segment, fused FK + boolean fields).  Needs the MI355X: there is no CPU path.

    python examples/plan_trajectories.py [--batch 256] [--horizon 64] [--iters 200] [--fused] [--via-cost N]
                                         [--model links|spheres|grasp|both]

--fused runs the same problem with the whole loop on the chip (`task.rollout_adam_plan(...).step(32)`, `trk_rollout_gp_adam_steps`):
trajectories and Adam's state stay in registers, one launch per 32 iterations (horizons that are a power of two up to 64).
--via-cost N (horizons up to 64) adds the collision cost at N via points per segment -- the configurations the validation judges
and the optimiser otherwise never sees -- and prints the collision-free count of both runs (the problem is solved twice for that).
In the eager loop it is one more launch per iteration (`task.rollout_via_plan`, `trk_rollout_via_cost_grad`: its gradient arrives
at the way points, same weight as the way points' own cost).  With --fused the term is part of the planning-loop kernel
(`task.rollout_adam_plan(..., w_via=1 / N, num_interpolation=N)`, `trk_rollout_gp_via_adam_steps`): the N via points of a segment
together weigh as much as one way point.
--model chooses the Panda's collision geometry: `links` (default: the link origins), `spheres` (the 45 link spheres), `grasp` (a
grasped box) or `both`.  For the three attached-point models an evaluation is `task.rollout_plan` (`trk_rollout_points_cost_grad`)
plus `ops.gp_prior_cost_grad`, and --fused is `task.points_adam_plan(...).step(32)` (`trk_rollout_points_gp_adam_steps`); the
via-point cost is not available for them (--via-cost is refused).
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra
from torch_robotics_amd import ops


MODELS = ("links", "spheres", "grasp", "both")


def make_robot(model, ta):
    """the Panda with the collision geometry --model names"""
    if model not in MODELS:
        raise ValueError(f"--model must be one of {', '.join(MODELS)}")
    kw = {}
    if model in ("spheres", "both"):
        kw["link_sphere_model"] = "panda"
    if model in ("grasp", "both"):
        kw["grasped_object"] = tra.GraspedObjectPandaBox(tensor_args=ta)
    return tra.RobotPanda(tensor_args=ta, **kw)


def main(batch=256, horizon=64, iters=200, device="cuda:0", verbose=True, seed=0, fused=False, stats=None, via_cost=0, model="links"):
    points = model != "links"
    if points and via_cost > 0:
        raise NotImplementedError("--via-cost is for --model links: the via-point cost kernels serve link-column cost models only")
    if via_cost > 0:                       # the same problem (same seed) without the via-point term first, for the comparison
        n_free_plain = main(batch, horizon, iters, device, False, seed, fused=fused)[1]
    torch.manual_seed(seed)
    ta = dict(device=torch.device(device), dtype=torch.float32)
    robot = make_robot(model, ta)
    # clamp_sdf=True: the fields are hinges relu(margin - sdf) (distance_fields.py:114-117) -- what an optimiser needs; the plain
    # margin - sdf that the reference's PlanningTask sums decreases without bound away from the obstacles
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=robot, obstacle_cutoff_margin=0.05, clamp_sdf=True,
                            tensor_args=ta)
    T, dt = 5.0, 5.0 / horizon
    q_start = task.random_coll_free_q(n_samples=1).reshape(1, 1, -1)
    q_goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, -1)
    s = torch.linspace(0.0, 1.0, horizon, **ta).reshape(1, horizon, 1)
    q = (q_start + s * (q_goal - q_start)).contiguous()                  # (B, H, D) straight lines in configuration space
    qd = ((q_goal - q_start) / T).expand(batch, horizon, -1).contiguous()

    w_obj, sigma_gp, lr = 50.0, 2.0, 1e-2
    if fused:
        res = _main_fused(task, q, qd, q_start + s * (q_goal - q_start), dt, sigma_gp, w_obj, lr, iters, verbose, stats, via_cost, points)
        if via_cost > 0:
            if stats is not None:
                stats.update(n_free_plain=n_free_plain, n_free_via=res[1])
            if verbose:
                print(f"collision-free without the via-point cost: {n_free_plain}/{batch}   with it ({via_cost} per segment, "
                      f"w_via = 1/{via_cost}): {res[1]}/{batch}")
        return res
    # pre-bound launch: reads q, qd in place; cost = w_obj * (self + object + workspace hinges) + the prior's factor costs
    if points:                             # attached points: the collision rollout pre-bound, the prior a call of its own per iteration
        plan = task.rollout_plan(q, w_self=w_obj, w_obj=w_obj, w_ws=w_obj, want_pos=False)
    else:
        plan = task.rollout_gp_plan(q, qd, dt, sigma_gp, gp_weight=1.0, w_self=w_obj, w_obj=w_obj, w_ws=w_obj)
    # the collision hinges at via_cost via points per segment, same weights: one more launch, its gradient lands on the way points
    via = task.rollout_via_plan(q, via_cost, w_self=w_obj, w_obj=w_obj, w_ws=w_obj) if via_cost > 0 else None
    free_mask = torch.ones(1, horizon, 1, **ta)
    free_mask[:, 0] = 0.0
    free_mask[:, -1] = 0.0                                               # start and goal stay fixed
    opt = torch.optim.Adam([q, qd], lr=lr)                               # the GP prior is stiff (1/dt^3): plain descent diverges
    hist = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        plan.launch()                                                    # plan.cost (B,H), plan.gq, plan.gqd (B,H,D)
        if points:                                                       # the prior from the SAME q / qd the launch read
            c_gp, gp_gq, gp_gqd = ops.gp_prior_cost_grad(q, qd, dt, sigma_gp)
            if verbose and (it % 50 == 0 or it == iters - 1):
                hist.append((it, float(plan.cost.sum(1).mean()) / w_obj, float(c_gp.mean())))
            q.grad = free_mask * (plan.gq + gp_gq)
            qd.grad = gp_gqd
            opt.step()
            continue
        if verbose and (it % 50 == 0 or it == iters - 1):
            # the prior's share of plan.cost, from the SAME q / qd the launch read (before the step moves them in place)
            c_gp = ops.gp_prior_cost_grad(q, qd, dt, sigma_gp)[0]
            hist.append((it, float((plan.cost.sum(1) - c_gp).mean()) / w_obj, float(c_gp.mean())))
        if via is not None:
            via.launch()
            q.grad = free_mask * (plan.gq + via.gq)
        else:
            q.grad = free_mask * plan.gq                                 # gradients come from the kernel, not from autograd
        qd.grad = plan.gqd
        opt.step()                                                       # in place: the plan keeps reading q's and qd's buffers
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    coll0 = task.compute_collision(q_start + s * (q_goal - q_start)).any(1).float().mean().item()
    trajs_coll, trajs_free = task.get_trajs_collision_and_free(q, num_interpolation=5)
    n_free = 0 if trajs_free is None else trajs_free.shape[0]
    if verbose:
        for it, c, g in hist:
            print(f"iter {it:4d}: mean collision cost per trajectory {c:9.4f}   mean GP-prior cost {g:9.4f}")
        print(f"{iters} iterations x {batch * horizon} configurations in {elapsed * 1e3:.1f} ms "
              f"({batch * horizon * iters / elapsed:.3g} FK+cost+grad evaluations/s incl. the Python loop)")
        print(f"straight lines in collision: {coll0 * 100:.0f} %   collision-free after optimisation: {n_free}/{batch}")
        if via is not None:
            print(f"collision-free without the via-point cost: {n_free_plain}/{batch}   with it ({via_cost} per segment): {n_free}/{batch}")
    return q, n_free, coll0


def _main_fused(task, q, qd, q_lines, dt, sigma_gp, w_obj, lr, iters, verbose, stats, via_cost=0, points=False):
    """the same objective, pins and Adam, `iters` iterations in launches of 32: plan.step(n) returns the cost of the state it started from"""
    batch, horizon = q.shape[:2]
    via = dict(w_via=1.0 / via_cost, num_interpolation=via_cost) if via_cost > 0 else {}
    make_plan = task.points_adam_plan if points else task.rollout_adam_plan      # attached points: their own planning-loop kernel
    plan = make_plan(q, qd, dt, sigma_gp, gp_weight=1.0, w_self=w_obj, w_obj=w_obj, w_ws=w_obj, lr=lr, **via)   # start and goal pinned
    probe = make_plan(q, qd, dt, sigma_gp, gp_weight=0.0, w_self=w_obj, w_obj=w_obj, w_ws=w_obj, lr=0.0)   # collision cost only
    cost0 = float(probe.step(1).sum(1).mean()) / w_obj
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < iters:
        n = min(32, iters - done)
        plan.step(n)
        done += n
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    cost1 = float(probe.step(1).sum(1).mean()) / w_obj
    coll0 = task.compute_collision(q_lines).any(1).float().mean().item()
    trajs_coll, trajs_free = task.get_trajs_collision_and_free(q, num_interpolation=5)
    n_free = 0 if trajs_free is None else trajs_free.shape[0]
    if stats is not None:
        stats.update(cost_before=cost0, cost_after=cost1, elapsed=elapsed)
    if verbose:
        print(f"mean collision cost per trajectory {cost0:9.4f} -> {cost1:9.4f}")
        print(f"{iters} fused iterations x {batch * horizon} configurations in {elapsed * 1e3:.1f} ms "
              f"({batch * horizon * iters / elapsed:.3g} FK+cost+grad+Adam evaluations/s)")
        print(f"straight lines in collision: {coll0 * 100:.0f} %   collision-free after optimisation: {n_free}/{batch}")
    return q, n_free, coll0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--fused", action="store_true", help="the whole loop in one kernel (rollout_adam_plan)")
    ap.add_argument("--via-cost", type=int, default=0, help="N > 0: add the collision cost at N via points per segment")
    ap.add_argument("--model", choices=MODELS, default="links", help="the Panda's collision geometry (default: link origins)")
    a = ap.parse_args()
    if a.model != "links" and a.via_cost > 0:
        ap.error("--via-cost is for --model links: the via-point cost kernels serve link-column cost models only")
    main(a.batch, a.horizon, a.iters, a.device, fused=a.fused, via_cost=a.via_cost, model=a.model)

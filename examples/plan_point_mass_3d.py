#!/usr/bin/env python3
"""Batch trajectory optimisation of the 3-D point mass in EnvSpheres3D, the 3-D sibling of examples/plan_point_mass_2d.py.

B straight lines between B starts and B goals (all sampled collision free) are improved by Adam on
    w_obj * sum_h (object + workspace hinge)  +  constant-velocity GP prior on (q, qd)
where the collision hinge is `PlanningTask(clamp_sdf=True).compute_collision_cost` and the prior is `ops.gp_prior_cost_grad`.  The
fraction of collision-free trajectories (`get_trajs_collision_and_free`: 5 via points per segment) is reported before and after.
Needs the MI355X: there is no CPU path.

    python examples/plan_point_mass_3d.py [--batch 512] [--horizon 64] [--iters 300] [--fused] [--via-cost N]

--fused runs the same problem through `task.point_mass_3d_optimizer`: the hinge, the prior, the pins and Adam in one kernel that keeps
the trajectories and the optimiser's state in registers, one launch per 32 iterations (`trk_point3d_traj_adam_steps`).

--via-cost N adds the hinge at the N via points of every segment -- with N = 5 the very points the reported fraction is judged at.  The
N via points of a segment together weigh as much as one way point: w_via = 1 / N on top of the objective's own w_obj.  With --fused the
term rides in the same kernel; without it, `task.compute_collision_cost_via(q, N)` joins the torch loop.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra
from torch_robotics_amd import ops

LAST = {}           # the summed clamped hinge cost of the batch before and after the latest main(): {"cost_before", "cost_after"}


def _free_fraction(task, q, qd):
    _, trajs_free = task.get_trajs_collision_and_free(torch.cat([q, qd], -1).detach())
    return 0.0 if trajs_free is None else trajs_free.shape[0] / q.shape[0]


def main(batch=512, horizon=64, iters=300, verbose=True, fused=False, via_cost=0, device="cuda:0", seed=0):
    torch.manual_seed(seed)
    ta = dict(device=torch.device(device), dtype=torch.float32)
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=tra.RobotPointMass3D(tensor_args=ta), obstacle_cutoff_margin=0.03,
                            clamp_sdf=True, tensor_args=ta)
    T, dt = 5.0, 5.0 / horizon
    start = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, 3)
    goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, 3)
    s = torch.linspace(0.0, 1.0, horizon, **ta).reshape(1, horizon, 1)
    q = (start + s * (goal - start)).contiguous().requires_grad_(not fused)
    qd = ((goal - start) / T).expand(batch, horizon, -1).contiguous().requires_grad_(not fused)
    before = _free_fraction(task, q, qd)
    LAST["cost_before"] = float(task.compute_collision_cost(q.detach()).sum())
    w_obj, sigma, lr = 20.0, 1.0, 5e-3
    w_via = 1.0 / via_cost if via_cost > 0 else 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if fused:
        # the loop below on the chip: same objective, same pins (start and goal positions), same Adam.  The kernel's via term is
        # w_via x the WEIGHTED hinge, so w_via = 1 / N there is w_obj / N here.
        plan = task.point_mass_3d_optimizer(q, qd, dt, sigma, w_obj=w_obj, w_ws=w_obj, lr=lr, w_via=w_via, num_interpolation=via_cost)
        plan.step(iters)
    else:
        opt = torch.optim.Adam([q, qd], lr=lr)
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            loss = w_obj * task.compute_collision_cost(q).sum()             # (B, H) hinge: relu(margin - sdf) + workspace
            if via_cost > 0:                                                # (B, (H-1) N) hinge at the via points, gradient on the way points
                loss = loss + w_obj * w_via * task.compute_collision_cost_via(q, via_cost).sum()
            loss.backward()
            _, gq, gqd = ops.gp_prior_cost_grad(q.detach(), qd.detach(), dt, sigma)
            q.grad.add_(gq)
            qd.grad = gqd                                                   # only the prior depends on qd
            q.grad[:, 0].zero_(); q.grad[:, -1].zero_()                     # start and goal stay where they are
            opt.step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    after = _free_fraction(task, q, qd)
    LAST["cost_after"] = float(task.compute_collision_cost(q.detach()).sum())
    if verbose:
        via = f", {via_cost} via points per segment in the objective" if via_cost > 0 else ""
        print(f"EnvSpheres3D, {batch} trajectories x {horizon} steps{', fused' if fused else ''}{via}: fraction of free trajectories "
              f"{before:.3f} -> {after:.3f}, summed hinge cost {LAST['cost_before']:.4g} -> {LAST['cost_after']:.4g} after {iters} Adam "
              f"iterations ({1e3 * elapsed / iters:.3f} ms / iteration)")
    return before, after


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--fused", action="store_true", help="the whole loop in one kernel (task.point_mass_3d_optimizer)")
    ap.add_argument("--via-cost", type=int, default=0, metavar="N", help="add the hinge at N via points per segment to the objective")
    a = ap.parse_args()
    b, f = main(a.batch, a.horizon, a.iters, fused=a.fused, via_cost=a.via_cost)
    sys.exit(0 if f >= b else 1)

#!/usr/bin/env python3
"""Batch trajectory optimisation of the 2-D point mass on EnvDense2D -- the standard benchmark of the motion-planning papers the
reference cites (MPOT, motion-planning diffusion), on the 2-D kernels of this package.

B straight lines from one start to B goals (both sampled collision free) are improved by Adam on
    w_obj * sum_h (object + workspace hinge)  +  constant-velocity GP prior on (q, qd)
where the collision hinge is `PlanningTask(clamp_sdf=True).compute_collision_cost` (one launch, the gradient written by the same
kernel) and the prior is `ops.gp_prior_cost_grad`.  The fraction of collision-free trajectories (`compute_fraction_free_trajs`: 5 via
points per segment, interpolated and tested in one launch) is reported before and after.  Needs the MI355X: there is no CPU path.

    python examples/plan_point_mass_2d.py [--batch 512] [--horizon 64] [--iters 300] [--fused] [--via-cost N]

--fused runs the same problem through `task.trajectory_optimizer`: the hinge, the prior, the pins and Adam in one kernel that keeps the
trajectories and the optimiser's state in registers, one launch per 32 iterations (`trk_scene2d_traj_adam_steps`).

--via-cost N adds the hinge at the N via points of every segment -- with N = 5 the very points the reported fraction is judged at -- so
that an obstacle between two way points costs the optimiser something.  The N via points of a segment together weigh as much as one way
point: w_via = w_obj / N, which keeps the collision term's scale against the prior whatever N is.  With --fused the term rides in the
same kernel (`trk_scene2d_traj_via_adam_steps`); without it, `task.compute_collision_cost_via(q, N)` joins the torch loop.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra
from torch_robotics_amd import ops


def main(batch=512, horizon=64, iters=300, device="cuda:0", verbose=True, seed=0, fused=False, via_cost=0):
    torch.manual_seed(seed)
    ta = dict(device=torch.device(device), dtype=torch.float32)
    env = tra.EnvDense2D(tensor_args=ta)
    task = tra.PlanningTask(env=env, robot=tra.RobotPointMass(tensor_args=ta), obstacle_cutoff_margin=0.02, clamp_sdf=True, tensor_args=ta)
    T, dt = 5.0, 5.0 / horizon
    start = task.random_coll_free_q(n_samples=1).reshape(1, 1, 2)
    goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, 2)
    s = torch.linspace(0.0, 1.0, horizon, **ta).reshape(1, horizon, 1)
    q = (start + s * (goal - start)).contiguous().requires_grad_(not fused)
    qd = ((goal - start) / T).expand(batch, horizon, -1).contiguous().requires_grad_(not fused)
    before = task.compute_fraction_free_trajs(torch.cat([q, qd], -1).detach())
    w_obj, sigma = 20.0, 1.0
    w_via = w_obj / via_cost if via_cost > 0 else 0.0
    if fused:
        return _main_fused(task, q, qd, dt, sigma, w_obj, iters, before, verbose, w_via, via_cost)
    opt = torch.optim.Adam([q, qd], lr=5e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        opt.zero_grad(set_to_none=True)
        cost = task.compute_collision_cost(q)                           # (B, H) hinge: relu(margin - sdf) + workspace
        loss = w_obj * cost.sum()
        if via_cost > 0:                                                # (B, (H-1) N) hinge at the via points, gradient on the way points
            loss = loss + w_via * task.compute_collision_cost_via(q, via_cost).sum()
        loss.backward()
        _, gq, gqd = ops.gp_prior_cost_grad(q.detach(), qd.detach(), dt, sigma)
        q.grad.add_(gq)
        qd.grad = gqd                                                   # only the prior depends on qd
        q.grad[:, 0].zero_(); q.grad[:, -1].zero_()                     # start and goal stay where they are
        opt.step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    trajs = torch.cat([q, qd], -1).detach()
    after = task.compute_fraction_free_trajs(trajs)
    if verbose:
        print(f"EnvDense2D, {batch} trajectories x {horizon} steps{_via_note(via_cost)}: fraction of free trajectories {before:.3f} -> {after:.3f} "
              f"after {iters} Adam iterations ({1e3 * elapsed / iters:.2f} ms / iteration)")
    return before, after


def _via_note(via_cost):
    return f", {via_cost} via points per segment in the objective" if via_cost > 0 else ""


def _main_fused(task, q, qd, dt, sigma, w_obj, iters, before, verbose, w_via=0.0, via_cost=0):
    """the loop of main() on the chip: same objective, same pins (start and goal positions), same Adam"""
    plan = task.trajectory_optimizer(q, qd, dt, sigma, w_obj=w_obj, lr=5e-3, w_via=w_via, num_interpolation=via_cost)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan.step(iters)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    after = task.compute_fraction_free_trajs(torch.cat([q, qd], -1))
    if verbose:
        print(f"EnvDense2D, {q.shape[0]} trajectories x {q.shape[1]} steps, fused{_via_note(via_cost)}: fraction of free trajectories {before:.3f} -> {after:.3f} "
              f"after {iters} Adam iterations ({1e3 * elapsed / iters:.3f} ms / iteration)")
    return before, after


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--fused", action="store_true", help="the whole loop in one kernel (task.trajectory_optimizer)")
    ap.add_argument("--via-cost", type=int, default=0, metavar="N", help="add the hinge at N via points per segment to the objective")
    a = ap.parse_args()
    b, f = main(a.batch, a.horizon, a.iters, fused=a.fused, via_cost=a.via_cost)
    sys.exit(0 if f > b else 1)

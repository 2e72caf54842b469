#!/usr/bin/env python3
"""Sampling-based planning (STOMP / MPPI style) at a horizon the Adam loops refuse: every problem starts from the straight line
between a collision-free start and goal, and `task.sampling_optimizer` improves it without a gradient -- perturb the mean with
GP-smooth noise (`trk_gp_prior_sample`), evaluate every particle, weight the particles by a soft-min of their costs
(`trk_traj_softmin_weights`), move the mean to the weighted particle mean (`trk_traj_weighted_update`).  The number of free
trajectories (`get_trajs_collision_and_free`) is printed before and after.
Needs the MI355X: there is no CPU path.

    python examples/plan_sampling.py [--robot panda|point3d] [--problems 64] [--horizon 128] [--particles 32] [--iters 100]
                                     [--mode trajectory|waypoint] [--seed 0]

--mode trajectory: MPPI's weights exp(-(S_k - min S) / lambda) of the particles' summed costs;
--mode waypoint: STOMP's probabilities per way point, exp(-h (c - min) / (max - min)) with h = 1 / lambda = 10.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra


def _setup(robot, ta):
    """-> (task, sigma_gp, sigma_noise, w_coll, gp_weight, the temperature of the trajectory mode)"""
    if robot == "panda":
        task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=tra.RobotPanda(tensor_args=ta), obstacle_cutoff_margin=0.05,
                                clamp_sdf=True, tensor_args=ta)
        return task, 2.0, 0.4, 50.0, 1.0, 1.0
    if robot == "point3d":
        task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=tra.RobotPointMass3D(tensor_args=ta),
                                obstacle_cutoff_margin=0.03, clamp_sdf=True, tensor_args=ta)
        return task, 1.0, 0.2, 20.0, 1.0, 1.0
    raise ValueError(f"robot must be 'panda' or 'point3d', got {robot!r}")


def _free(task, q, qd):
    return int(task.get_trajs_collision_and_free(torch.cat([q, qd], -1), return_indices=True)[3].numel())


def main(robot="panda", problems=64, horizon=128, particles=32, iters=100, mode="trajectory", device="cuda:0", seed=0, verbose=True):
    torch.manual_seed(seed)
    ta = dict(device=torch.device(device), dtype=torch.float32)
    task, sigma_gp, sigma_noise, w_coll, gp_weight, lam = _setup(robot, ta)
    T, dt = 5.0, 5.0 / horizon
    D = task.robot.q_dim
    start = task.random_coll_free_q(n_samples=problems).reshape(problems, D)
    goal = task.random_coll_free_q(n_samples=problems).reshape(problems, D)
    s = torch.linspace(0.0, 1.0, horizon, **ta).reshape(1, horizon, 1)
    q = (start[:, None] + s * (goal - start)[:, None]).contiguous()
    qd = ((goal - start) / T)[:, None].expand(problems, horizon, D).contiguous()
    before = _free(task, q, qd)
    gen = torch.Generator(device=ta["device"]).manual_seed(seed)
    plan = task.sampling_optimizer(q, qd, dt, sigma_gp, particles, sigma_noise, lam if mode == "trajectory" else 0.1, mode=mode,
                                   w_coll=w_coll, gp_weight=gp_weight, generator=gen)
    first = plan.step(iters)
    after = _free(task, q, qd)
    if verbose:
        last = plan.cost(q, qd).sum(1)
        print(f"{robot}, EnvSpheres3D, {problems} problems x {horizon} steps, {particles} particles, {iters} iterations, mode {mode}: "
              f"{before}/{problems} straight lines free, {after}/{problems} free afterwards; mean cost {float(first.mean()):.3f} -> "
              f"{float(last.mean()):.3f}")
    return before, after


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", choices=("panda", "point3d"), default="panda")
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--particles", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--mode", choices=("trajectory", "waypoint"), default="trajectory")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    main(a.robot, a.problems, a.horizon, a.particles, a.iters, a.mode, seed=a.seed)

#!/usr/bin/env python3
"""Multi-particle planning: the same problems planned from ONE straight line each and from several particles each drawn from the
start/goal-conditioned GP prior (`task.sample_gp_trajs`, `trk_gp_prior_sample`), both through the planning loop on the chip, then
the best collision-free particle per problem is kept (`task.select_best_trajs`, `trk_traj_select_best`).

A descent from one line stays in that line's basin; particles from the prior the loop already carries as a cost start in several.
Particle 0 of a problem is the prior's mean (zero noise: the straight line at constant velocity), the others are drawn at a sigma
chosen for their spread: conditioned on start and goal, the prior's standard deviation half way is sigma sqrt(T^3 / 48) -- 3.2 rad for
the arm at the loop's own sigma = 2 and T = 5 s, wider than the joint ranges -- so the draw uses sigma_init = spread / sqrt(T^3 / 48)
with `--spread` (default 0.3 rad for the arm, 0.15 m for the point mass) as the standard deviation half way.
Needs the MI355X: there is no CPU path.

    python examples/plan_particles.py [--problems 64] [--particles 8] [--horizon 64] [--iters 200] [--model links|point3d] [--spread S]
                                      [--resample S]

--model links: the Panda in EnvSpheres3D through `task.rollout_adam_plan` (horizons 2, 4, ..., 64);
--model point3d: the 3-D point mass in EnvSpheres3D through `task.point_mass_3d_optimizer` (horizons up to 256).
--resample S: the winners are resampled to S points by the clamped cubic spline through their way points (`tra.smoothen_trajectory`,
`trk_traj_spline_resample`) and validated again; both free counts and the winners' way-point variance
(`tra.compute_variance_waypoints`, `trk_traj_waypoint_variance`) are printed.  Off by default: the output is unchanged without it.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra


def _setup(model, ta):
    """-> (task, make_plan(q, qd, dt) -> plan, the default spread of the particles half way)"""
    if model == "links":
        task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=tra.RobotPanda(tensor_args=ta), obstacle_cutoff_margin=0.05,
                                clamp_sdf=True, tensor_args=ta)
        w, sigma, lr = 50.0, 2.0, 1e-2
        return task, (lambda q, qd, dt: task.rollout_adam_plan(q, qd, dt, sigma, gp_weight=1.0, w_self=w, w_obj=w, w_ws=w, lr=lr)), 0.3
    if model == "point3d":
        task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=ta), robot=tra.RobotPointMass3D(tensor_args=ta),
                                obstacle_cutoff_margin=0.03, clamp_sdf=True, tensor_args=ta)
        w, sigma, lr = 20.0, 1.0, 5e-3
        return task, (lambda q, qd, dt: task.point_mass_3d_optimizer(q, qd, dt, sigma, w_obj=w, w_ws=w, lr=lr)), 0.15
    raise ValueError(f"model must be 'links' or 'point3d', got {model!r}")


def _plan_and_pick(task, make_plan, q, qd, dt, iters, particles, winners=False):
    """the planning loop on (q, qd) in place, then the winner of every problem -> number of problems solved (and the winners)"""
    make_plan(q, qd, dt).step(iters)
    best, _, solved = task.select_best_trajs(torch.cat([q, qd], -1), particles)
    return (int(solved.sum()), best) if winners else int(solved.sum())


def _resample_and_validate(task, best, n_points):
    """the winners (P, H, 2 D) resampled to n_points way points -> (free before, free after, the way-point variance of the winners)"""
    D = task.robot.q_dim
    free = lambda trajs: int(task.get_trajs_collision_and_free(trajs, return_indices=True)[3].numel())
    pos, vel = tra.smoothen_trajectory(best[..., :D].contiguous(), n_support_points=n_points, set_average_velocity=False)
    dense = torch.cat([pos, vel], -1)
    return free(best), free(dense), float(tra.compute_variance_waypoints(best, task.robot))


def main(problems=64, particles=8, horizon=64, iters=200, model="links", device="cuda:0", seed=0, verbose=True, spread=None, resample=0):
    torch.manual_seed(seed)
    ta = dict(device=torch.device(device), dtype=torch.float32)
    task, make_plan, default_spread = _setup(model, ta)
    T, dt = 5.0, 5.0 / horizon
    D = task.robot.q_dim
    start = task.random_coll_free_q(n_samples=problems).reshape(problems, D)
    goal = task.random_coll_free_q(n_samples=problems).reshape(problems, D)
    # one straight line per problem at constant velocity
    s = torch.linspace(0.0, 1.0, horizon, **ta).reshape(1, horizon, 1)
    q = (start[:, None] + s * (goal - start)[:, None]).contiguous()
    qd = ((goal - start) / T)[:, None].expand(problems, horizon, D).contiguous()
    solved_line = _plan_and_pick(task, make_plan, q, qd, dt, iters, 1)
    # `particles` draws per problem from the prior between the same start and goal, the first of them its mean
    sigma_init = (default_spread if spread is None else spread) / (T ** 3 / 48.0) ** 0.5
    gen = torch.Generator(device=ta["device"]).manual_seed(seed)
    eps = torch.randn((problems * particles, horizon - 1, D, 2), generator=gen, **ta)
    eps[::particles] = 0.0
    qp, qdp = task.sample_gp_trajs(start, goal, particles, horizon, dt, sigma_init, eps=eps)
    solved_particles, best = _plan_and_pick(task, make_plan, qp, qdp, dt, iters, particles, winners=True)
    if verbose:
        print(f"{model}, EnvSpheres3D, {problems} problems x {horizon} steps, {iters} Adam iterations: solved {solved_line}/{problems} "
              f"from one straight line each, {solved_particles}/{problems} from {particles} GP-prior particles each (sigma_init "
              f"{sigma_init:.3f})")
    if resample:
        free_before, free_after, variance = _resample_and_validate(task, best, resample)
        if verbose:
            print(f"winners resampled {horizon} -> {resample} points by the clamped cubic spline: {free_before}/{problems} free before, "
                  f"{free_after}/{problems} after; way-point variance of the winners {variance:.4f}")
        return solved_line, solved_particles, free_before, free_after, variance
    return solved_line, solved_particles


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--particles", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--model", choices=("links", "point3d"), default="links")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spread", type=float, default=None, help="standard deviation of the particles half way (rad / m)")
    ap.add_argument("--resample", type=int, default=0, help="resample the winners to this many points and validate them again")
    a = ap.parse_args()
    main(a.problems, a.particles, a.horizon, a.iters, a.model, seed=a.seed, spread=a.spread, resample=a.resample)

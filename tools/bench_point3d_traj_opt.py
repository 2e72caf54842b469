#!/usr/bin/env python3
"""The planning loop of the 3-D point mass on the MI355X: the eager loop that examples/plan_point_mass_3d.py runs without --fused
(`task.compute_collision_cost(q).sum().backward()`, `ops.gp_prior_cost_grad`, the pins and `torch.optim.Adam.step()` per iteration)
against the fused loop of `Point3DAdamPlan.step(32)` (trk_point3d_traj_adam_steps, kernel k_point3d_traj), on EnvSpheres3D and
EnvTableShelf with the example's weights, at 256 x 64 and 4096 x 64.

    python tools/bench_point3d_traj_opt.py [--iters 320] [--repeats 5] [--via-cost N] [--json out.json]

Wall time per iteration = host clock around `iters` iterations ending in a device synchronise, the median [min, max] of `repeats`
windows, the arms alternating in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch

import torch_robotics_amd as tra
from bench_arm_traj_opt import BATCHES, TA, problem, window
from torch_robotics_amd import ops

SCENES = ("EnvSpheres3D", "EnvTableShelf")
H, W_OBJ, SIGMA, LR = 64, 20.0, 1.0, 5e-3          # the example's
DT = 5.0 / H


def make_task(scene):
    return tra.PlanningTask(env=getattr(tra, scene)(tensor_args=TA), robot=tra.RobotPointMass3D(tensor_args=TA), obstacle_cutoff_margin=0.03,
                            clamp_sdf=True, tensor_args=TA)


class Unfused:
    """the example's eager loop, one iteration per pass"""

    def __init__(self, task, q, qd, via_cost):
        self.task, self.via_cost = task, via_cost
        self.q, self.qd = q.clone().requires_grad_(True), qd.clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        q, qd, task = self.q, self.qd, self.task
        for _ in range(iters):
            self.opt.zero_grad(set_to_none=True)
            loss = W_OBJ * task.compute_collision_cost(q).sum()
            if self.via_cost > 0:
                loss = loss + (W_OBJ / self.via_cost) * task.compute_collision_cost_via(q, self.via_cost).sum()
            loss.backward()
            _, gq, gqd = ops.gp_prior_cost_grad(q.detach(), qd.detach(), DT, SIGMA)
            q.grad.add_(gq)
            qd.grad = gqd
            q.grad[:, 0].zero_(); q.grad[:, -1].zero_()
            self.opt.step()


class Fused:
    def __init__(self, task, q, qd, via_cost):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.point_mass_3d_optimizer(self.q, self.qd, DT, SIGMA, w_obj=W_OBJ, w_ws=W_OBJ, lr=LR,
                                                 w_via=1.0 / via_cost if via_cost > 0 else 0.0, num_interpolation=via_cost)

    def run(self, iters):
        for _ in range(iters // 32):
            self.plan.step(32)
        if iters % 32:
            self.plan.step(iters % 32)


ARMS = dict(unfused=Unfused, fused=Fused)


def main(iters, repeats, warmup, via_cost, out):
    rows = []
    for scene in SCENES:
        task = make_task(scene)
        for batch in BATCHES:
            q, qd = problem(task, batch)
            arms = {k: cls(task, q, qd, via_cost) for k, cls in ARMS.items()}
            for arm in arms.values():
                arm.run(warmup)
            ts = {k: [] for k in arms}
            for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
                for k, arm in arms.items():
                    ts[k].append(window(arm, iters))
            row = dict(scene=scene, robot="RobotPointMass3D", shape=f"{batch} x {H}", via_points_per_segment=via_cost, iters_per_window=iters,
                       repeats=repeats)
            for k, v in ts.items():
                row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
                row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            spread = sum(max(v) - min(v) for v in ts.values())
            row["combined_window_spread_us"] = round(spread, 3)
            row["gain_us_per_iter"] = round(row["unfused_us_per_iter"] - row["fused_us_per_iter"], 3)
            row["fused_is_faster_beyond_the_spread"] = bool(row["gain_us_per_iter"] > spread)
            row["loop_speedup"] = round(row["unfused_us_per_iter"] / row["fused_us_per_iter"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--via-cost", type=int, default=0, metavar="N", help="the hinge also at N via points per segment, in both arms")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    main(a.iters, a.repeats, a.warmup, a.via_cost, a.json)

#!/usr/bin/env python3
"""The planning loop of the Panda's attached-point models on the MI355X: the eager loop of examples/plan_trajectories.py --model
spheres | grasp | both (one `PointsRolloutPlan.launch()`, `ops.gp_prior_cost_grad`, the mask multiply and `torch.optim.Adam.step()`
per iteration) against the fused loop of `PointsAdamPlan.step(32)` (trk_rollout_points_gp_adam_steps, kernel k_padam), on
EnvSpheres3D with the example's weights, at 256 x 64 and 4096 x 64; `evaluation` is one `PointsRolloutPlan.launch()` alone.

    python tools/bench_points_traj_opt.py [--iters 320] [--repeats 5] [--json out.json]      wall times, every model and size
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_points_traj_opt.py --trace ARM --model MODEL --case BATCH --iters 96
        one arm (unfused | fused | evaluation) of one case and nothing after it
    python tools/bench_points_traj_opt.py --summarize DIR --iters 96 --tail 64
        that trace's kernel time per iteration (tools/bench_arm_traj_opt.py's summary)

Wall time per iteration = host clock around `iters` iterations ending in a device synchronise, the median of `repeats` windows, the
arms alternating in one process."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch

import torch_robotics_amd as tra
from bench_arm_traj_opt import BATCHES, DT, H, LR, SIGMA, TA, W_OBJ, problem, summarize, window
from torch_robotics_amd import ops

MODELS = ("spheres", "grasp", "both")


def make_task(model):
    kw = {}
    if model in ("spheres", "both"):
        kw["link_sphere_model"] = "panda"
    if model in ("grasp", "both"):
        kw["grasped_object"] = tra.GraspedObjectPandaBox(tensor_args=TA)
    return tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=tra.RobotPanda(tensor_args=TA, **kw), obstacle_cutoff_margin=0.05,
                            clamp_sdf=True, tensor_args=TA)


class Unfused:
    """the example's eager loop for a point model, one iteration per pass"""

    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_plan(self.q, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ, want_pos=False)
        self.mask = torch.ones(1, H, 1, **TA)
        self.mask[:, 0] = 0.0
        self.mask[:, -1] = 0.0
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()
            _, gq, gqd = ops.gp_prior_cost_grad(self.q, self.qd, DT, SIGMA)
            self.q.grad = self.mask * (self.plan.gq + gq)
            self.qd.grad = gqd
            self.opt.step()


class Fused:
    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.points_adam_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ, lr=LR)

    def run(self, iters):
        for _ in range(iters // 32):
            self.plan.step(32)
        if iters % 32:
            self.plan.step(iters % 32)


class Evaluation:
    """one PointsRolloutPlan.launch() per pass: the collision objective and its gradient, no prior, no update"""

    def __init__(self, task, q, qd):
        self.q = q.clone()
        self.plan = task.rollout_plan(self.q, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ, want_pos=False)

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()


ARMS = dict(unfused=Unfused, fused=Fused, evaluation=Evaluation)


def main(iters, repeats, warmup, out):
    rows = []
    for model in MODELS:
        task = make_task(model)
        for batch in BATCHES:
            q, qd = problem(task, batch)
            arms = {k: cls(task, q, qd) for k, cls in ARMS.items()}
            for arm in arms.values():
                arm.run(warmup)
            ts = {k: [] for k in arms}
            for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
                for k, arm in arms.items():
                    ts[k].append(window(arm, iters))
            row = dict(scene="EnvSpheres3D", robot=f"RobotPanda ({model})", shape=f"{batch} x {H}", iters_per_window=iters, repeats=repeats)
            for k, v in ts.items():
                row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
                row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            spread = sum(max(ts[k]) - min(ts[k]) for k in ("unfused", "fused"))
            row["combined_window_spread_us"] = round(spread, 3)
            row["gain_us_per_iter"] = round(row["unfused_us_per_iter"] - row["fused_us_per_iter"], 3)
            row["fused_is_faster_beyond_the_spread"] = bool(row["gain_us_per_iter"] > spread)
            row["loop_speedup"] = round(row["unfused_us_per_iter"] / row["fused_us_per_iter"], 2)
            row["fused_over_one_evaluation"] = round(row["fused_us_per_iter"] / row["evaluation_us_per_iter"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


def trace(which, iters, model, case):
    task = make_task(model)
    for batch in BATCHES:
        if case and str(case) != str(batch):
            continue
        q, qd = problem(task, batch)
        ARMS[which](task, q, qd).run(iters)
        torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", choices=sorted(ARMS), default=None)
    ap.add_argument("--model", choices=MODELS, default="grasp", help="--trace: the model")
    ap.add_argument("--case", default=None, help="BATCH, e.g. 256 (--trace)")
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    ap.add_argument("--tail", type=int, default=64)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters, a.tail, loop_kernels=("k_padam",))
    elif a.trace:
        trace(a.trace, a.iters, a.model, a.case)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

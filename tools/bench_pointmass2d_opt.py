#!/usr/bin/env python3
"""The 2-D point mass's planning loop on the MI355X: examples/plan_point_mass_2d.py's loop of separate launches (hinge + autograd,
GP prior, gradient fix-ups, torch.optim.Adam) against the fused loop of `PlanarAdamPlan.step(32)` (trk_scene2d_traj_adam_steps), and
`planar_traj_cost_grad` alone against the hinge and prior launches it replaces.

    python tools/bench_pointmass2d_opt.py [--iters 320] [--repeats 5] [--json out.json]      wall times, every case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_pointmass2d_opt.py --trace ARM --case SCENE:BATCH --iters 96
        one arm (unfused | fused | objective | objective2) of one case and nothing after it
    python tools/bench_pointmass2d_opt.py --summarize DIR --iters 96 --tail 64
        that trace's kernel time per iteration: the dispatches of the last `tail` iterations are the end of the trace, a whole number
        of repeats of one iteration's kernel sequence (found as the trace's period), so set-up and first-iteration kernels stay out

Cases: EnvDense2D (grid) and EnvNarrowPassageDense2D (analytic), 512 x 64 and 4096 x 64.  Wall time per iteration = host clock
around `iters` iterations ending in a device synchronise, the median of `repeats` windows, the arms alternating."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra
from torch_robotics_amd import ops

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
SCENES = ("EnvDense2D", "EnvNarrowPassageDense2D")
BATCHES = (512, 4096)
H, W_OBJ, SIGMA, LR = 64, 20.0, 1.0, 5e-3
DT = 5.0 / H


def problem(task, batch, seed=0):
    torch.manual_seed(seed)
    start = task.random_coll_free_q(n_samples=1).reshape(1, 1, 2)
    goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, 2)
    s = torch.linspace(0.0, 1.0, H, **TA).reshape(1, H, 1)
    return (start + s * (goal - start)).contiguous(), ((goal - start) / 5.0).expand(batch, H, -1).contiguous()


class Unfused:
    """the example's loop, one iteration per call of step()"""

    def __init__(self, task, q, qd):
        self.task, self.q, self.qd = task, q.clone().requires_grad_(True), qd.clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        q, qd = self.q, self.qd
        for _ in range(iters):
            self.opt.zero_grad(set_to_none=True)
            (W_OBJ * self.task.compute_collision_cost(q).sum()).backward()
            _, gq, gqd = ops.gp_prior_cost_grad(q.detach(), qd.detach(), DT, SIGMA)
            q.grad.add_(gq)
            qd.grad = gqd
            q.grad[:, 0].zero_(); q.grad[:, -1].zero_()
            self.opt.step()


class Fused:
    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.trajectory_optimizer(self.q, self.qd, DT, SIGMA, w_obj=W_OBJ, lr=LR)

    def run(self, iters):
        for _ in range(iters // 32):
            self.plan.step(32)
        if iters % 32:
            self.plan.step(iters % 32)


class Objective:
    """one evaluation of the objective and its gradients: the fused launch, or the hinge and the prior as launches of their own"""

    def __init__(self, task, q, qd, fused):
        self.scene, self.clamp = task._planar_handles(DEV)
        self.q, self.qd, self.fused = q, qd, fused

    def run(self, iters):
        for _ in range(iters):
            if self.fused:
                ops.planar_traj_cost_grad(self.scene, self.q, self.qd, DT, SIGMA, 1.0, W_OBJ, self.clamp)
            else:
                ops.planar_cost_grad(self.scene, self.q, clamp=self.clamp)
                ops.gp_prior_cost_grad(self.q, self.qd, DT, SIGMA)


def window(arm, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arm.run(iters)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def tasks():
    for name in SCENES:
        yield name, tra.PlanningTask(env=getattr(tra, name)(tensor_args=TA), robot=tra.RobotPointMass(tensor_args=TA),
                                     obstacle_cutoff_margin=0.02, clamp_sdf=True, tensor_args=TA)


def main(iters, repeats, warmup, out):
    rows = []
    for name, task in tasks():
        for batch in BATCHES:
            q, qd = problem(task, batch)
            arms = dict(unfused=Unfused(task, q, qd), fused=Fused(task, q, qd), objective_two_launches=Objective(task, q, qd, False),
                        objective_fused=Objective(task, q, qd, True))
            for arm in arms.values():
                arm.run(warmup)
            early = float((arms["unfused"].q.detach() - arms["fused"].q).abs().max())
            ts = {k: [] for k in arms}
            for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
                for k, arm in arms.items():
                    ts[k].append(window(arm, iters))
            # same problem, same arithmetic up to rounding: the two loops must stay together
            drift = float((arms["unfused"].q.detach() - arms["fused"].q).abs().max())
            row = dict(scene=name, shape=f"{batch} x {H}", iters_per_window=iters, repeats=repeats, max_abs_q_difference_after_warmup=early,
                       max_abs_q_difference_between_loops=drift)
            for k, v in ts.items():
                row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
                row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row["loop_speedup"] = round(row["unfused_us_per_iter"] / row["fused_us_per_iter"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


def trace(which, iters, case):
    for name, task in tasks():
        for batch in BATCHES:
            if case and case != f"{name}:{batch}":
                continue
            q, qd = problem(task, batch)
            arm = {"unfused": lambda: Unfused(task, q, qd), "fused": lambda: Fused(task, q, qd),
                   "objective": lambda: Objective(task, q, qd, True), "objective2": lambda: Objective(task, q, qd, False)}[which]()
            arm.run(iters)
            torch.cuda.synchronize()


def summarize(trace_dir, iters, tail):
    """kernel time per iteration of the last `tail` of `iters` iterations of a --trace run, from rocprofv3's kernel_trace.csv"""
    import csv
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        rows += list(csv.DictReader(f.open()))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    fused = any("k_planar_traj_adam" in n for n in names[-20:])
    per_launch = 32 if fused else 1                                                 # the fused loop: 32 iterations per launch
    groups = tail // per_launch
    if fused:                                                                       # one kernel per 32 iterations: its last launches, by name
        loop = [r for r in rows if "k_planar_traj_adam" in r["Kernel_Name"]][-groups:]
        ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in loop)
        out = dict(trace=str(trace_dir), kernels_per_iteration=1 / per_launch, kernel_us_per_iteration=round(ns / 1e3 / (len(loop) * per_launch), 3),
                   kernels={loop[-1]["Kernel_Name"][:90]: 1})
        print(json.dumps(out), flush=True)
        return out
    for drop in range(0, 17):                                                       # the runtime's own copies at process exit follow the loop
        end = len(names) - drop
        for k in range(1, end // max(1, groups) + 1):                               # the period: kernels per group
            t = names[end - groups * k:end]
            if not all(t[i] == t[i + k] for i in range(len(t) - k)):
                continue
            loop = rows[end - groups * k:end]
            ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in loop)
            by = {}
            for r in loop[:k]:
                by[r["Kernel_Name"][:90]] = by.get(r["Kernel_Name"][:90], 0) + 1
            out = dict(trace=str(trace_dir), kernels_per_iteration=k / per_launch, kernel_us_per_iteration=round(ns / 1e3 / (groups * per_launch), 3),
                       kernels=by)
            print(json.dumps(out), flush=True)
            return out
    raise SystemExit(f"{trace_dir}: no periodic tail of {groups} groups found in {len(names)} dispatches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", choices=["unfused", "fused", "objective", "objective2"], default=None)
    ap.add_argument("--case", default=None, help="SCENE:BATCH, e.g. EnvDense2D:512 (--trace)")
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    ap.add_argument("--tail", type=int, default=64)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters, a.tail)
    elif a.trace:
        trace(a.trace, a.iters, a.case)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

#!/usr/bin/env python3
"""The Panda's planning loop on the MI355X: examples/plan_trajectories.py's loop (one `RolloutGpPlan.launch()`, a mask multiply and
`torch.optim.Adam.step()` per iteration) against the fused loop of `ArmAdamPlan.step(32)` (trk_rollout_gp_adam_steps), on EnvSpheres3D
with the example's weights, at 256 x 64 and 4096 x 64; `evaluation` is one `RolloutGpPlan.launch()` alone.

    python tools/bench_arm_traj_opt.py [--iters 320] [--repeats 5] [--json out.json]      wall times, every case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_arm_traj_opt.py --trace ARM --case BATCH --iters 96
        one arm (unfused | fused | evaluation) of one case and nothing after it
    python tools/bench_arm_traj_opt.py --summarize DIR --iters 96 --tail 64
        that trace's kernel time per iteration (the periodic tail of the trace, as tools/bench_pointmass2d_opt.py finds it)

Wall time per iteration = host clock around `iters` iterations ending in a device synchronise, the median of `repeats` windows, the
arms alternating."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
BATCHES = (256, 4096)
H, W_OBJ, SIGMA, LR = 64, 50.0, 2.0, 1e-2
DT = 5.0 / H


def make_task():
    return tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05,
                            clamp_sdf=True, tensor_args=TA)


def problem(task, batch, seed=0):
    torch.manual_seed(seed)
    start = task.random_coll_free_q(n_samples=1).reshape(1, 1, -1)
    goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, -1)
    s = torch.linspace(0.0, 1.0, H, **TA).reshape(1, H, 1)
    return (start + s * (goal - start)).contiguous(), ((goal - start) / 5.0).expand(batch, H, -1).contiguous()


class Unfused:
    """the example's loop, one iteration per pass"""

    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_gp_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ)
        self.mask = torch.ones(1, H, 1, **TA)
        self.mask[:, 0] = 0.0
        self.mask[:, -1] = 0.0
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()
            self.q.grad = self.mask * self.plan.gq
            self.qd.grad = self.plan.gqd
            self.opt.step()


class Fused:
    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_adam_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ, lr=LR)

    def run(self, iters):
        for _ in range(iters // 32):
            self.plan.step(32)
        if iters % 32:
            self.plan.step(iters % 32)


class Evaluation:
    """one RolloutGpPlan.launch() per pass: the objective and its gradients, no update"""

    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_gp_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ)

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()


ARMS = dict(unfused=Unfused, fused=Fused, evaluation=Evaluation)


def window(arm, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arm.run(iters)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main(iters, repeats, warmup, out):
    task, rows = make_task(), []
    for batch in BATCHES:
        q, qd = problem(task, batch)
        arms = {k: cls(task, q, qd) for k, cls in ARMS.items()}
        for arm in arms.values():
            arm.run(warmup)
        ts = {k: [] for k in arms}
        for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
            for k, arm in arms.items():
                ts[k].append(window(arm, iters))
        row = dict(scene="EnvSpheres3D", robot="RobotPanda", shape=f"{batch} x {H}", iters_per_window=iters, repeats=repeats)
        for k, v in ts.items():
            row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
            row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        row["loop_speedup"] = round(row["unfused_us_per_iter"] / row["fused_us_per_iter"], 2)
        row["fused_over_one_evaluation"] = round(row["fused_us_per_iter"] / row["evaluation_us_per_iter"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


def trace(which, iters, case):
    task = make_task()
    for batch in BATCHES:
        if case and str(case) != str(batch):
            continue
        q, qd = problem(task, batch)
        ARMS[which](task, q, qd).run(iters)
        torch.cuda.synchronize()


def summarize(trace_dir, iters, tail, loop_kernels=("k_traj_adam",)):
    """kernel time per iteration of the last `tail` of `iters` iterations of a --trace run, from rocprofv3's kernel_trace.csv;
    loop_kernels: the names that mark a trace of a fused loop (tools/bench_arm_traj_via.py adds its own)"""
    import csv
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        rows += list(csv.DictReader(f.open()))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    is_loop = lambda n: any(k in n for k in loop_kernels)
    fused = any(is_loop(n) for n in names[-20:])
    per_launch = 32 if fused else 1                                                 # the fused loop: 32 iterations per launch
    groups = tail // per_launch
    if fused:                                                                       # one kernel per 32 iterations: its last launches, by name
        loop = [r for r in rows if is_loop(r["Kernel_Name"])][-groups:]
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
    ap.add_argument("--trace", choices=sorted(ARMS), default=None)
    ap.add_argument("--case", default=None, help="BATCH, e.g. 256 (--trace)")
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    ap.add_argument("--tail", type=int, default=64)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters, a.tail)
    elif a.trace:
        trace(a.trace, a.iters, a.case)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

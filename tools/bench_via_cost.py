#!/usr/bin/env python3
"""The via-point collision cost and its way-point gradient on the MI355X: the fused launch (`RolloutViaPlan.launch()`,
trk_rollout_via_cost_grad) against the two-step route -- `ops.interpolate_traj_via_points`, `ops.rollout_cost_grad` on the
materialised via points, the gradient folded back onto the way points with torch -- for the Panda on EnvSpheres3D at 256 x 64 x 5 and
4096 x 64 x 5.  The two-step route uses nothing the fused kernel brought: it is what the package could do before.

    python tools/bench_via_cost.py [--iters 200] [--repeats 5] [--json out.json]      wall times, both cases
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_via_cost.py --trace ARM --case BATCH --iters 64
        one arm (fused | two_step) of one case and nothing after it
    python tools/bench_via_cost.py --summarize DIR --iters 64 --case BATCH
        that trace's kernel time per evaluation (the periodic tail of the trace: the last 32 evaluations)

Wall time per evaluation = host clock around `iters` evaluations ending in a device synchronise, the median [min, max] of `repeats`
windows, the arms alternating."""
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
BATCHES = (256, 4096)
H, N = 64, 5
W = (1.0, 1.0, 1.0, 0.0)


def make_task():
    return tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05,
                            clamp_sdf=True, tensor_args=TA)


def problem(task, batch, seed=0):
    torch.manual_seed(seed)
    start = task.random_coll_free_q(n_samples=1).reshape(1, 1, -1)
    goal = task.random_coll_free_q(n_samples=batch).reshape(batch, 1, -1)
    s = torch.linspace(0.0, 1.0, H, **TA).reshape(1, H, 1)
    return (start + s * (goal - start)).contiguous()


class Fused:
    def __init__(self, task, x):
        model, cm = task._fused_handles(DEV)
        self.plan = ops.RolloutViaPlan(model, cm, W, x.clone(), N)
        self.cost, self.gq = self.plan.cost, self.plan.gq

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()


class TwoStep:
    """interpolate, roll out on (H - 1) n configurations per trajectory, fold: the buffers of the rollout are allocated once"""

    def __init__(self, task, x):
        self.model, self.cm = task._fused_handles(DEV)
        self.x = x.clone()
        T, D = x.shape[0], x.shape[2]
        self.alpha, self.beta = (v.reshape(1, 1, N, 1) for v in ops.via_point_weights(N, DEV))
        self.cost = torch.empty((T, (H - 1) * N), **TA)
        self.g = torch.empty((T, (H - 1) * N, D), **TA)
        self.gq = torch.zeros((T, H, D), **TA)

    def run(self, iters):
        T, D = self.x.shape[0], self.x.shape[2]
        for _ in range(iters):
            v = ops.interpolate_traj_via_points(self.x, N)
            ops.rollout_cost_grad(self.model, self.cm, W, v, want_pos=False, out=(None, self.cost, self.g))
            g4 = self.g.view(T, H - 1, N, D)
            self.gq.zero_()
            self.gq[:, :-1] += (g4 * self.alpha).sum(2)
            self.gq[:, 1:] += (g4 * self.beta).sum(2)


ARMS = dict(fused=Fused, two_step=TwoStep)


def window(arm, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arm.run(iters)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main(iters, repeats, warmup, out):
    task, rows = make_task(), []
    for batch in BATCHES:
        x = problem(task, batch)
        arms = {k: cls(task, x) for k, cls in ARMS.items()}
        for arm in arms.values():
            arm.run(warmup)
        torch.cuda.synchronize()
        agree = float((arms["fused"].gq - arms["two_step"].gq).abs().max() / arms["two_step"].gq.abs().max())
        ts = {k: [] for k in arms}
        for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
            for k, arm in arms.items():
                ts[k].append(window(arm, iters))
        row = dict(scene="EnvSpheres3D", robot="RobotPanda", shape=f"{batch} x {H} x {N}", via_points=batch * (H - 1) * N,
                   iters_per_window=iters, repeats=repeats, gq_max_rel_diff=agree)
        for k, v in ts.items():
            row[f"{k}_us"] = round(statistics.median(v), 3)
            row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        spread = sum(max(v) - min(v) for v in ts.values())
        row["margin_us"] = round(row["two_step_us"] - row["fused_us"], 3)
        row["spread_us"] = round(spread, 3)
        row["fused_wins_beyond_spread"] = bool(row["margin_us"] > spread)
        row["speedup"] = round(row["two_step_us"] / row["fused_us"], 2)
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
        ARMS[which](task, problem(task, batch)).run(iters)
        torch.cuda.synchronize()


def summarize(trace_dir, iters, case, tail=32):
    """kernel time per evaluation over the last `tail` of `iters` evaluations of a --trace run, from rocprofv3's kernel_trace.csv: the
    periodic tail of the dispatch sequence (as tools/bench_arm_traj_opt.py finds it); for the rollout-family kernel also the time per
    sample (via point)"""
    import csv
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        rows += list(csv.DictReader(f.open()))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    samples = int(case) * (H - 1) * N
    for drop in range(0, 17):                                                       # the runtime's own copies at process exit follow the loop
        end = len(names) - drop
        for k in range(1, end // max(1, tail) + 1):                                 # the period: kernels per evaluation
            t = names[end - tail * k:end]
            if not all(t[i] == t[i + k] for i in range(len(t) - k)):
                continue
            loop = rows[end - tail * k:end]
            by = {}
            for r in loop:
                e = by.setdefault(r["Kernel_Name"], [0, 0])
                e[0] += 1
                e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            out = dict(trace=str(trace_dir), kernels_per_evaluation=k,
                       kernel_us_per_evaluation=round(sum(v[1] for v in by.values()) / 1e3 / tail, 3),
                       kernels={n[:80]: dict(per_evaluation=v[0] // tail, us=round(v[1] / 1e3 / v[0], 3)) for n, v in by.items()})
            for n, v in by.items():
                if "k_via_cost" in n or "k_rollout" in n:
                    out["rollout_family_kernel"] = n[:80]
                    out["ns_per_via_point"] = round(v[1] / v[0] / samples, 5)
            print(json.dumps(out), flush=True)
            return out
    raise SystemExit(f"{trace_dir}: no periodic tail of {tail} evaluations found in {len(names)} dispatches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", choices=sorted(ARMS), default=None)
    ap.add_argument("--case", default=None, help="BATCH, e.g. 256 (--trace, --summarize)")
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters, a.case or BATCHES[-1])
    elif a.trace:
        trace(a.trace, a.iters, a.case)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

#!/usr/bin/env python3
"""The Panda's planning loop WITH the via-point term on the MI355X, on EnvSpheres3D with the example's weights and 5 via points per
segment, at 256 x 64 and 4096 x 64.  Three arms, alternating in one process:

    fused_via   `ArmAdamPlan(..., w_via=1 / 5, num_interpolation=5).step(32)` (trk_rollout_gp_via_adam_steps, kernel k_traj_via_adam)
    fused       the same plan without the term (trk_rollout_gp_adam_steps, k_traj_adam): what the term costs inside the kernel
    eager_via   examples/plan_trajectories.py --via-cost 5: `RolloutGpPlan.launch()`, `RolloutViaPlan.launch()`, the mask multiply
                and `torch.optim.Adam.step()` per iteration

    python tools/bench_arm_traj_via.py [--iters 320] [--repeats 5] [--json out.json]      wall times, every case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_arm_traj_via.py --trace ARM --case BATCH --iters 96
        one arm of one case and nothing after it
    python tools/bench_arm_traj_via.py --summarize DIR --iters 96 --tail 64
        that trace's kernel time per iteration (tools/bench_arm_traj_opt.py's reading of the trace's periodic tail)

Wall time per iteration = host clock around `iters` iterations ending in a device synchronise, the median [min, max] of `repeats`
windows.  `fused_via_beats_eager_via_beyond_spread`: the gap between the two medians exceeds the two arms' spreads (max - min) added."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch

import bench_arm_traj_opt as base
from bench_arm_traj_opt import BATCHES, DT, H, LR, SIGMA, TA, W_OBJ

N_VIA = 5
W_VIA = 1.0 / N_VIA


class FusedVia(base.Fused):
    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_adam_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ, lr=LR,
                                           w_via=W_VIA, num_interpolation=N_VIA)


class EagerVia:
    """the example's loop with --via-cost, one iteration per pass"""

    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.rollout_gp_plan(self.q, self.qd, DT, SIGMA, gp_weight=1.0, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ)
        self.via = task.rollout_via_plan(self.q, N_VIA, w_self=W_OBJ, w_obj=W_OBJ, w_ws=W_OBJ)
        self.mask = torch.ones(1, H, 1, **TA)
        self.mask[:, 0] = 0.0
        self.mask[:, -1] = 0.0
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        for _ in range(iters):
            self.plan.launch()
            self.via.launch()
            self.q.grad = self.mask * (self.plan.gq + self.via.gq)
            self.qd.grad = self.plan.gqd
            self.opt.step()


ARMS = dict(fused_via=FusedVia, fused=base.Fused, eager_via=EagerVia)


def main(iters, repeats, warmup, out):
    task, rows = base.make_task(), []
    for batch in BATCHES:
        q, qd = base.problem(task, batch)
        arms = {k: cls(task, q, qd) for k, cls in ARMS.items()}
        for arm in arms.values():
            arm.run(warmup)
        ts = {k: [] for k in arms}
        for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
            for k, arm in arms.items():
                ts[k].append(base.window(arm, iters))
        row = dict(scene="EnvSpheres3D", robot="RobotPanda", shape=f"{batch} x {H}", n_via=N_VIA, w_via=W_VIA, iters_per_window=iters,
                   repeats=repeats)
        for k, v in ts.items():
            row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
            row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        spread = sum(max(ts[k]) - min(ts[k]) for k in ("fused_via", "eager_via"))
        row["eager_via_over_fused_via"] = round(row["eager_via_us_per_iter"] / row["fused_via_us_per_iter"], 2)
        row["fused_via_over_fused"] = round(row["fused_via_us_per_iter"] / row["fused_us_per_iter"], 2)
        row["combined_spread_us"] = round(spread, 3)
        row["fused_via_beats_eager_via_beyond_spread"] = bool(row["eager_via_us_per_iter"] - row["fused_via_us_per_iter"] > spread)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


def trace(which, iters, case):
    task = base.make_task()
    for batch in BATCHES:
        if case and str(case) != str(batch):
            continue
        q, qd = base.problem(task, batch)
        ARMS[which](task, q, qd).run(iters)
        torch.cuda.synchronize()


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
        base.summarize(a.summarize, a.iters, a.tail, loop_kernels=("k_traj_adam", "k_traj_via_adam"))
    elif a.trace:
        trace(a.trace, a.iters, a.case)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

#!/usr/bin/env python3
"""The 2-D point mass's planning loop WITH the via-point collision term on the MI355X, three arms on one problem:
  unfused    the example's torch loop with the two-step via cost: compute_collision_cost + compute_collision_cost_via (interpolate,
             k_planar_cost on the materialised points, the gradient folded back by torch launches) + gp_prior_cost_grad + torch.optim.Adam
  fused      `PlanarAdamPlan.step(32)` without the via term (trk_scene2d_traj_adam_steps) -- what the via term is priced against
  fused_via  `PlanarAdamPlan.step(32)` with it (trk_scene2d_traj_via_adam_steps)

    python tools/bench_pointmass2d_via.py [--iters 320] [--repeats 5] [--json out.json]      wall times, every case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_pointmass2d_via.py --trace ARM --case SCENE:BATCH --iters 96
        one arm of one case and nothing after it
    python tools/bench_pointmass2d_via.py --summarize DIR --iters 96 --tail 64
        that trace's kernel time per iteration (tools/bench_pointmass2d_opt.py's rule: the periodic tail of the trace)
    python tools/bench_pointmass2d_via.py --free-fraction [--iters 300]
        the fraction of collision-free trajectories at 512 x 64 after `iters` fused iterations, with and without the via term

Cases: EnvDense2D (grid) and EnvNarrowPassageDense2D (analytic), 512 x 64 and 4096 x 64, n = 5 via points per segment weighed as in
examples/plan_point_mass_2d.py (w_via = w_obj / n).  Wall time per iteration = host clock around `iters` iterations ending in a device
synchronise, the median of `repeats` windows, the arms alternating."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch

import bench_pointmass2d_opt as base
from bench_pointmass2d_opt import BATCHES, DT, H, LR, SIGMA, W_OBJ
from torch_robotics_amd import ops

N_VIA = 5
W_VIA = W_OBJ / N_VIA


class UnfusedVia:
    """the example's loop with --via-cost, one iteration per call"""

    def __init__(self, task, q, qd):
        self.task, self.q, self.qd = task, q.clone().requires_grad_(True), qd.clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.q, self.qd], lr=LR)

    def run(self, iters):
        q, qd = self.q, self.qd
        for _ in range(iters):
            self.opt.zero_grad(set_to_none=True)
            (W_OBJ * self.task.compute_collision_cost(q).sum() + W_VIA * self.task.compute_collision_cost_via(q, N_VIA).sum()).backward()
            _, gq, gqd = ops.gp_prior_cost_grad(q.detach(), qd.detach(), DT, SIGMA)
            q.grad.add_(gq)
            qd.grad = gqd
            q.grad[:, 0].zero_(); q.grad[:, -1].zero_()
            self.opt.step()


class FusedVia(base.Fused):
    def __init__(self, task, q, qd):
        self.q, self.qd = q.clone(), qd.clone()
        self.plan = task.trajectory_optimizer(self.q, self.qd, DT, SIGMA, w_obj=W_OBJ, lr=LR, w_via=W_VIA, num_interpolation=N_VIA)


ARMS = dict(unfused=UnfusedVia, fused=base.Fused, fused_via=FusedVia)


def main(iters, repeats, warmup, out):
    rows = []
    for name, task in base.tasks():
        for batch in BATCHES:
            q, qd = base.problem(task, batch)
            arms = {k: cls(task, q, qd) for k, cls in ARMS.items()}
            for arm in arms.values():
                arm.run(warmup)
            ts = {k: [] for k in arms}
            for _ in range(repeats):                                 # alternating, so that drift hits every arm alike
                for k, arm in arms.items():
                    ts[k].append(base.window(arm, iters))
            # same problem, same objective up to rounding: the two via loops must stay together
            drift = float((arms["unfused"].q.detach() - arms["fused_via"].q).abs().max())
            row = dict(scene=name, shape=f"{batch} x {H}", n_via=N_VIA, iters_per_window=iters, repeats=repeats,
                       max_abs_q_difference_between_via_loops=drift)
            for k, v in ts.items():
                row[f"{k}_us_per_iter"] = round(statistics.median(v), 3)
                row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row["via_loop_speedup"] = round(row["unfused_us_per_iter"] / row["fused_via_us_per_iter"], 1)
            row["price_of_the_via_term"] = round(row["fused_via_us_per_iter"] / row["fused_us_per_iter"], 2)
            spread = lambda k: max(ts[k]) - min(ts[k])
            row["fused_via_below_unfused_by_more_than_both_spreads"] = bool(
                row["unfused_us_per_iter"] - row["fused_via_us_per_iter"] > spread("unfused") + spread("fused_via"))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))


def trace(which, iters, case):
    for name, task in base.tasks():
        for batch in BATCHES:
            if case and case != f"{name}:{batch}":
                continue
            q, qd = base.problem(task, batch)
            ARMS[which](task, q, qd).run(iters)
            torch.cuda.synchronize()


def summarize(trace_dir, iters, tail):
    """base.summarize, which knows the loop kernel of the plain fused arm by name; the via loop's kernel is k_planar_traj_via"""
    import csv
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        rows += list(csv.DictReader(f.open()))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    loop = [r for r in rows if "k_planar_traj_via" in r["Kernel_Name"]]
    if not loop:
        return base.summarize(trace_dir, iters, tail)
    loop = loop[-(tail // 32):]
    ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in loop)
    out = dict(trace=str(trace_dir), kernels_per_iteration=1 / 32, kernel_us_per_iteration=round(ns / 1e3 / (len(loop) * 32), 3),
               kernels={loop[-1]["Kernel_Name"][:90]: 1})
    print(json.dumps(out), flush=True)
    return out


def free_fraction(iters, batch=512):
    rows = []
    for name, task in base.tasks():
        q0, qd0 = base.problem(task, batch)
        row = dict(scene=name, shape=f"{batch} x {H}", iters=iters, before=task.compute_fraction_free_trajs(torch.cat([q0, qd0], -1)))
        for key, kw in (("without_via", {}), ("with_via", dict(w_via=W_VIA, num_interpolation=N_VIA))):
            q, qd = q0.clone(), qd0.clone()
            task.trajectory_optimizer(q, qd, DT, SIGMA, w_obj=W_OBJ, lr=LR, **kw).step(iters)
            row[key] = task.compute_fraction_free_trajs(torch.cat([q, qd], -1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", choices=sorted(ARMS), default=None)
    ap.add_argument("--case", default=None, help="SCENE:BATCH, e.g. EnvDense2D:512 (--trace)")
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    ap.add_argument("--tail", type=int, default=64)
    ap.add_argument("--free-fraction", action="store_true")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters or 96, a.tail)
    elif a.trace:
        trace(a.trace, a.iters or 96, a.case)
    elif a.free_fraction:
        free_fraction(a.iters or 300)
    else:
        main(a.iters or 320, a.repeats, a.warmup, a.json)

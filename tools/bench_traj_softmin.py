#!/usr/bin/env python3
"""The sampling-based trajectory update's two ops on the MI355X against the torch composition of the same result, written here:

  weights   `ops.traj_softmin_weights` (trk_traj_softmin_weights, one launch, trajectory mode) against
            `torch.softmax(-cost.double().sum(1).view(P, K) / lambda, 1).float()`;
  update    `ops.traj_weighted_update` (trk_traj_weighted_update, one launch up to 64 particles, two beyond) against
            `mean + (w.view(P, K, 1, 1) * (x.view(P, K, H, D) - mean[:, None])).sum(1)`;
  at (problems, particles, horizon, dim) = (512, 8, 64, 7), (512, 64, 64, 7), (1, 4096, 64, 7), (64, 32, 128, 14);
  plan      one whole iteration of `PlanningTask.sampling_optimizer` (the Panda in EnvSpheres3D, 64 problems x 32 particles x 128 way
            points) against the same iteration with the two ops replaced by the torch lines above -- the sampler, the clamp and the
            cost are the same calls in both arms.

    python tools/bench_traj_softmin.py [--iters 200] [--repeats 5] [--json out.json]

Wall time per call = host clock around `iters` calls ending in a device synchronise, the median [min, max] of `repeats` windows, the
two arms alternating in one process after a warm-up.  A negative gain means the torch arm won: it is reported as measured.  No kernel
time is taken here: an HBM fraction of the update (4 P K H C bytes) needs a `--kernel-trace` run of its own."""
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
SHAPES = ((512, 8, 64, 7), (512, 64, 64, 7), (1, 4096, 64, 7), (64, 32, 128, 14))
PLAN_SHAPE = (64, 32, 128)
LAMBDA = 1.0


def torch_weights(cost, P, K, lam):
    return torch.softmax(-cost.double().sum(1).view(P, K) / lam, 1).float().view(P * K)


def torch_update(mean, x, w, step):
    P, H, D = mean.shape
    K = x.shape[0] // P
    return mean + step * (w.view(P, K, 1, 1) * (x.view(P, K, H, D) - mean[:, None])).sum(1)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def compare(row, arms, iters, repeats, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in arms}
    for _ in range(repeats):                                     # alternating, so that drift hits both arms alike
        for k, fn in arms.items():
            ts[k].append(window(fn, iters))
    for k, v in ts.items():
        row[f"{k}_us_per_call"] = round(statistics.median(v), 3)
        row[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    spread = sum(max(v) - min(v) for v in ts.values())
    row["combined_window_spread_us"] = round(spread, 3)
    row["gain_us_per_call"] = round(row["torch_us_per_call"] - row["op_us_per_call"], 3)
    row["op_is_faster_beyond_the_spread"] = bool(row["gain_us_per_call"] > spread)
    row["torch_is_faster_beyond_the_spread"] = bool(-row["gain_us_per_call"] > spread)
    row["speedup"] = round(row["torch_us_per_call"] / row["op_us_per_call"], 2)
    row.update(iters_per_window=iters, repeats=repeats)
    print(json.dumps(row), flush=True)
    return row


def plan_arms(gen):
    """-> (arms, the plan): one iteration through the plan, and the same iteration with torch in place of the two ops"""
    P, K, H = PLAN_SHAPE
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=tra.RobotPanda(tensor_args=TA), obstacle_cutoff_margin=0.05,
                            clamp_sdf=True, tensor_args=TA)
    D = task.robot.q_dim
    torch.manual_seed(0)
    start = task.random_coll_free_q(n_samples=P).reshape(P, D)
    goal = task.random_coll_free_q(n_samples=P).reshape(P, D)
    s = torch.linspace(0.0, 1.0, H, **TA).reshape(1, H, 1)
    q0 = (start[:, None] + s * (goal - start)[:, None]).contiguous()
    qd0 = ((goal - start) / 5.0)[:, None].expand(P, H, D).contiguous()
    q, qd = q0.clone(), qd0.clone()
    plan = task.sampling_optimizer(q, qd, 5.0 / H, 2.0, K, 0.4, LAMBDA, w_coll=50.0, generator=gen)
    lo, hi = plan._lim

    def through_the_plan():
        q.copy_(q0), qd.copy_(qd0)
        plan.step(1)

    def in_torch():
        q.copy_(q0), qd.copy_(qd0)
        xq, xqd = plan.particles()
        c = plan.cost(xq, xqd)
        w = torch_weights(c, P, K, LAMBDA)
        nq = torch.minimum(torch.maximum(torch_update(q, xq, w, 1.0), lo), hi)
        nq[:, 0], nq[:, -1] = q[:, 0], q[:, -1]
        q.copy_(nq)
        qd.copy_(torch_update(qd, xqd, w, 1.0))

    return dict(op=through_the_plan, torch=in_torch), plan


def main(iters, repeats, warmup, out):
    rows = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for P, K, H, D in SHAPES:
        cost = torch.rand((P * K, H), generator=gen, **TA) * (4.0 / H)
        mean = torch.randn((P, H, D), generator=gen, **TA)
        x = (mean[:, None] + 0.3 * torch.randn((P, K, H, D), generator=gen, **TA)).reshape(P * K, H, D).contiguous()
        arms = dict(op=lambda: ops.traj_softmin_weights(cost, K, LAMBDA)[0], torch=lambda: torch_weights(cost, P, K, LAMBDA))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="traj_softmin_weights", shape=f"{P} x {K} x {H}", max_relative_difference=float(((a - b).abs() / b).max()))
        rows.append(compare(row, arms, iters, repeats, warmup))
        w = a
        arms = dict(op=lambda: ops.traj_weighted_update(mean, x, w, 1.0, 0), torch=lambda: torch_update(mean, x, w, 1.0))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="traj_weighted_update", shape=f"{P} x {K} x {H} x {D}", max_abs_difference=float((a - b).abs().max()),
                   bytes_of_x=4 * P * K * H * D)
        rows.append(compare(row, arms, iters, repeats, warmup))
    arms, _plan = plan_arms(gen)
    P, K, H = PLAN_SHAPE
    row = dict(op="sampling_optimizer.step(1)", shape=f"Panda, {P} x {K} x {H} x 7")
    rows.append(compare(row, arms, max(5, iters // 4), repeats, max(2, warmup // 4)))
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    main(a.iters, a.repeats, a.warmup, a.json)

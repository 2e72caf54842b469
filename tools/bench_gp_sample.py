#!/usr/bin/env python3
"""Multi-particle planning's two ops on the MI355X against the torch composition of the same result, written here:

  sampler  `ops.gp_prior_sample` (trk_gp_prior_sample, one launch) against the conditioned walk from `torch.cumsum`
           at (trajectories, horizon, dof) = (256, 64, 7), (4096, 64, 7), (4096, 256, 3), positions pinned, limits on;
  pick     `ops.traj_select_best` (trk_traj_select_best, one launch) against a masked `argmin`
           at (problems, particles) = (512, 8), (4096, 64).

    python tools/bench_gp_sample.py [--iters 200] [--repeats 5] [--json out.json]

Wall time per call = host clock around `iters` calls ending in a device synchronise, the median [min, max] of `repeats` windows, the
two arms alternating in one process after a warm-up.  The noise is made once, outside the windows, for both arms."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from torch_robotics_amd import ops

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
DT_T, SIGMA, K = 5.0, 2.0, 8
SAMPLE_SHAPES = ((256, 64, 7), (4096, 64, 7), (4096, 256, 3))
PICK_SHAPES = ((512, 8), (4096, 64))


def torch_sample(start, goal, eps, H, dt, sigma, K, q_min, q_max):
    """the positions-pinned draw of trk_gp_prior_sample from cumulative sums"""
    l00, l10, l11 = sigma * dt ** 1.5 / math.sqrt(3.0), sigma * (math.sqrt(3.0) / 2.0) * math.sqrt(dt), sigma * math.sqrt(dt) / 2.0
    st, go = start.repeat_interleave(K, 0), goal.repeat_interleave(K, 0)
    e0, e1 = eps[..., 0], eps[..., 1]
    zero = torch.zeros_like(st[:, None])
    v = torch.cat([zero, torch.cumsum(l10 * e0 + l11 * e1, 1)], 1)
    p = st[:, None] + torch.cat([zero, torch.cumsum(dt * v[:, :-1] + l00 * e0, 1)], 1)
    theta = (H - 1) * dt
    vs = (go - p[:, -1]) / theta
    t = torch.arange(H, **TA).reshape(1, H, 1)
    q = p + (t * dt) * vs[:, None]
    qd = v + vs[:, None]
    q[:, 1:-1] = torch.minimum(torch.maximum(q[:, 1:-1], q_min), q_max)
    q[:, 0], q[:, -1] = st, go
    return q, qd


def torch_pick(score, is_free, K):
    s = torch.where((is_free != 0) & ~torch.isnan(score), score, torch.full_like(score, float("inf"))).view(-1, K)
    bs, k = s.min(1)
    n_free = (is_free.view(-1, K) != 0).sum(1, dtype=torch.int32)
    has = ((is_free != 0) & ~torch.isnan(score)).view(-1, K).any(1)
    best = torch.where(has, k + torch.arange(s.shape[0], device=DEV) * K, torch.full_like(k, -1))
    return best, bs, n_free


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
    row["speedup"] = round(row["torch_us_per_call"] / row["op_us_per_call"], 2)
    row.update(iters_per_window=iters, repeats=repeats)
    print(json.dumps(row), flush=True)
    return row


def main(iters, repeats, warmup, out):
    rows = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N, H, D in SAMPLE_SHAPES:
        P, dt = N // K, DT_T / H
        start, goal = (torch.randn((P, D), generator=gen, **TA) for _ in range(2))
        eps = torch.randn((N, H - 1, D, 2), generator=gen, **TA)
        q_min, q_max = torch.full((D,), -2.5, **TA), torch.full((D,), 2.5, **TA)
        arms = dict(op=lambda: ops.gp_prior_sample(start, goal, H, dt, SIGMA, K, eps=eps, q_min=q_min, q_max=q_max),
                    torch=lambda: torch_sample(start, goal, eps, H, dt, SIGMA, K, q_min, q_max))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="gp_prior_sample", shape=f"{N} x {H} x {D}", particles=K,
                   max_abs_difference=float(max((a[0] - b[0]).abs().max(), (a[1] - b[1]).abs().max())))
        rows.append(compare(row, arms, iters, repeats, warmup))
    for P, Kp in PICK_SHAPES:
        score = torch.randn((P * Kp,), generator=gen, **TA)
        is_free = (torch.rand((P * Kp,), generator=gen, device=DEV) < 0.5).to(torch.uint8)
        arms = dict(op=lambda: ops.traj_select_best(score, is_free, Kp), torch=lambda: torch_pick(score, is_free, Kp))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="traj_select_best", shape=f"{P} x {Kp}", same_result=bool(all(torch.equal(x, y) for x, y in zip(a, b))))
        rows.append(compare(row, arms, iters, repeats, warmup))
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

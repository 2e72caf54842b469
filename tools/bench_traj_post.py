#!/usr/bin/env python3
"""Trajectory post-processing's two ops on the MI355X against the honest torch alternative, written here:

  spline    `ops.traj_spline_resample` (trk_traj_spline_resample, one launch, positions and the spline's derivative) against two
            `torch.matmul(W, y)`: the spline is linear in y, so W_pos and W_vel (S x N, formed in fp64 from the unit paths, rounded
            once) are precomputed outside the windows; at (trajectories, points, dim) -> samples = (256, 64, 7) -> 256 and
            (4096, 64, 7) -> 256;
  variance  `ops.traj_waypoint_variance` (trk_traj_waypoint_variance, two launches) against the reference's loop over the way points
            (`cdist`, `triu`, `var`) in torch on the GPU, at (problems, particles, horizon, dim) = (512, 8, 64, 7), (1, 4096, 64, 7).

    python tools/bench_traj_post.py [--iters 200] [--repeats 5] [--json out.json]

Wall time per call = host clock around `iters` calls ending in a device synchronise, the median [min, max] of `repeats` windows, the
two arms alternating in one process after a warm-up.  A negative gain means the torch arm won: it is reported as measured."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from torch_robotics_amd import ops

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
SPLINE_SHAPES = ((256, 64, 7, 256), (4096, 64, 7, 256))
VAR_SHAPES = ((512, 8, 64, 7), (1, 4096, 64, 7))


def spline_matrices(N, S):
    """W_pos, W_vel [S, N] in fp64: column j is the clamped spline through the unit path e_j, sampled (include/trk.h's arithmetic)"""
    y = np.eye(N)
    s = np.zeros((N, N))
    if N > 2:
        A = 4.0 * np.eye(N - 2) + np.eye(N - 2, k=1) + np.eye(N - 2, k=-1)
        s[1:-1] = np.linalg.solve(A, 3.0 * (N - 1) * (y[2:] - y[:-2]))
    a = np.arange(S) * (N - 1)
    i, r = a // (S - 1), a % (S - 1)
    i[-1], r[-1] = N - 2, S - 1
    tau = (r / (S - 1.0))[:, None]
    y0, y1, s0, s1 = y[i], y[i + 1], s[i], s[i + 1]
    W_pos = y0 + (3 * tau ** 2 - 2 * tau ** 3) * (y1 - y0) + tau * (1 - tau) * ((1 - tau) * s0 - tau * s1) / (N - 1)
    W_vel = (N - 1) * 6 * tau * (1 - tau) * (y1 - y0) + (1 - tau) * (1 - 3 * tau) * s0 + tau * (3 * tau - 2) * s1
    W_vel[0] = W_vel[-1] = 0.0
    return W_pos, W_vel


def torch_variance(trajs):
    """compute_variance_waypoints (trajectory/metrics.py:14-24, without its unused B x H x H matrix) per problem"""
    out = []
    for pos in trajs:
        total = 0.0
        for via_points in pos.permute(1, 0, 2):
            d = torch.cdist(via_points, via_points, p=2)
            total = total + torch.var(torch.triu(d, diagonal=1).view(-1))
        out.append(total)
    return torch.stack(out)


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


def main(iters, repeats, warmup, out):
    rows = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for n, N, D, S in SPLINE_SHAPES:
        y = torch.cumsum(0.3 * torch.randn((n, N, D), generator=gen, **TA), 1)
        W_pos, W_vel = (torch.as_tensor(w, dtype=torch.float32).to(DEV) for w in spline_matrices(N, S))
        arms = dict(op=lambda: ops.traj_spline_resample(y, S, "spline"), torch=lambda: (torch.matmul(W_pos, y), torch.matmul(W_vel, y)))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="traj_spline_resample", shape=f"{n} x {N} x {D} -> {S}",
                   max_abs_difference=[float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())])
        rows.append(compare(row, arms, iters, repeats, warmup))
    for P, K, H, D in VAR_SHAPES:
        x = torch.randn((P, K, H, D), generator=gen, **TA)
        slow = P * H > 4096                                       # the torch loop launches several kernels per (problem, way point)
        it, wu = (max(2, iters // 100), 1) if slow else (max(5, iters // 10), max(2, warmup // 10))
        arms = dict(op=lambda: ops.traj_waypoint_variance(x, 0, D), torch=lambda: torch_variance(x))
        a, b = arms["op"](), arms["torch"]()
        row = dict(op="traj_waypoint_variance", shape=f"{P} x {K} x {H} x {D}", max_relative_difference=float(((a - b).abs() / b.abs()).max()))
        rows.append(compare(row, arms, it, repeats, wu))
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

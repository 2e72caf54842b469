#!/usr/bin/env python3
"""The boolean path of the attached-point models on the MI355X: the fused kernel (k_pcoll: ops.rollout_points_collision[_via]) against
the two-step routing it replaces (fk_points + collision_fields; for validation the via points materialised first and the flags as a
launch of their own), for the Panda with the 45 link spheres, with the grasped box and with both on EnvSpheres3D:

    compute_collision            4096 x 64 configurations
    validation                   get_trajs_collision_and_free on 4096 x 64 trajectories, 5 via points per segment

The two arms are the same task under TRK_POINTS_COLLISION_FUSED = 1 / 0 (read per call), alternating in one process.

    python tools/bench_points_collision.py [--iters 10] [--repeats 5] [--json out.json]       wall times, every case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_points_collision.py --trace ARM --iters 10
        one arm (fused | two_step), every case, each between two separator launches (k_reduce_sum)
    python tools/bench_points_collision.py --summarize DIR --iters 10 [--stats out.txt]
        that trace's kernel time per call and the kernels of one call, case by case

Wall time per call = host clock around `iters` calls ending in a device synchronise, the median of `repeats` windows."""
import argparse
import json
import os
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
B, H, N_VIA = 4096, 64, 5
SWITCH = "TRK_POINTS_COLLISION_FUSED"
ARMS = dict(fused="1", two_step="0")
MODELS = {
    "spheres": lambda: tra.RobotPanda(link_sphere_model="panda", tensor_args=TA),
    "grasp": lambda: tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
    "spheres_grasp": lambda: tra.RobotPanda(link_sphere_model="panda", grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
}
CALLS = ("compute_collision", "validation")


def make_case(model):
    """(task, q (B, H, 7) uniform in the limits, trajectories (B, H, 7): short random walks off uniform starts)"""
    robot = MODELS[model]()
    task = tra.PlanningTask(env=tra.EnvSpheres3D(tensor_args=TA), robot=robot, obstacle_cutoff_margin=0.03, tensor_args=TA)
    gen = torch.Generator(device=DEV).manual_seed(0)
    q = robot.random_q(B * H, generator=gen).reshape(B, H, 7).contiguous()
    start = robot.random_q(B, generator=gen).reshape(B, 1, 7)
    trajs = start + 0.01 * torch.randn(B, H, 7, device=DEV, generator=gen).cumsum(1)
    trajs = torch.minimum(torch.maximum(trajs, robot.q_min.to(DEV)), robot.q_max.to(DEV)).contiguous()
    return task, q, trajs


def run(task, call, x, iters):
    for _ in range(iters):
        if call == "compute_collision":
            task.compute_collision(x)
        else:
            task.get_trajs_collision_and_free(x, return_indices=True, num_interpolation=N_VIA)


def window(task, call, x, arm, iters):
    os.environ[SWITCH] = ARMS[arm]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(task, call, x, iters)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main(iters, repeats, warmup, out):
    rows = []
    for model in MODELS:
        task, q, trajs = make_case(model)
        for call in CALLS:
            x = q if call == "compute_collision" else trajs
            for arm in ARMS:
                window(task, call, x, arm, warmup)
            served = {}
            for arm in ARMS:                                         # what served the arm's last launch of the rollout family
                window(task, call, x, arm, 1)
                served[arm] = ops.last_dispatch()
            ts = {arm: [] for arm in ARMS}
            for _ in range(repeats):                                 # alternating, so that drift hits both arms alike
                for arm in ARMS:
                    ts[arm].append(window(task, call, x, arm, iters))
            row = dict(scene="EnvSpheres3D", model=model, call=call, shape=f"{B} x {H}" + (f", {N_VIA} via points" if call == "validation" else ""),
                       iters_per_window=iters, repeats=repeats, fused_dispatch=served["fused"])
            for arm, v in ts.items():
                row[f"{arm}_us_per_call"] = round(statistics.median(v), 1)
                row[f"{arm}_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
            row["wall_speedup"] = round(row["two_step_us_per_call"] / row["fused_us_per_call"], 2)
            # the requirement: the fused arm is below the two-step arm by more than either arm's spread
            spread = max(max(v) - min(v) for v in ts.values())
            row["wall_gain_exceeds_spread"] = bool(row["two_step_us_per_call"] - row["fused_us_per_call"] > spread)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del task, q, trajs
        torch.cuda.empty_cache()
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(rows, indent=1) + "\n")


def separator():
    ops.reduce_sum(torch.zeros(8, **TA))


def trace(arm, iters, warmup):
    """every case of one arm: warm-up, a separator launch, `iters` calls, a separator launch"""
    os.environ[SWITCH] = ARMS[arm]
    for model in MODELS:
        task, q, trajs = make_case(model)
        for call in CALLS:
            x = q if call == "compute_collision" else trajs
            run(task, call, x, warmup)
            torch.cuda.synchronize()
            separator()
            run(task, call, x, iters)
            separator()
            torch.cuda.synchronize()
        del task, q, trajs
        torch.cuda.empty_cache()


def summarize(trace_dir, iters, stats):
    """kernel time per call of each case of a --trace run, from rocprofv3's kernel_trace.csv: the dispatches between the case's two
    separator launches"""
    import csv
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        rows += list(csv.DictReader(f.open()))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seps = [i for i, r in enumerate(rows) if "k_reduce_sum" in r["Kernel_Name"]]
    cases = [(m, c) for m in MODELS for c in CALLS]
    if len(seps) != 2 * len(cases):
        raise SystemExit(f"{trace_dir}: {len(seps)} separator launches, expected {2 * len(cases)}")
    out, lines = [], []
    for k, (model, call) in enumerate(cases):
        seg = rows[seps[2 * k] + 1:seps[2 * k + 1]]
        by = {}
        for r in seg:
            e = by.setdefault(r["Kernel_Name"][:100], [0, 0])
            e[0] += 1
            e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        total = sum(v[1] for v in by.values())
        rec = dict(trace=str(trace_dir), model=model, call=call, kernels_per_call=round(len(seg) / iters, 2),
                   kernel_us_per_call=round(total / 1e3 / iters, 2))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        lines.append(f"{model} / {call}: {rec['kernel_us_per_call']} us of kernel time per call, {rec['kernels_per_call']} launches per call")
        for name, (cnt, ns) in sorted(by.items(), key=lambda kv: -kv[1][1]):
            lines.append(f"    {ns / 1e3 / iters:12.2f} us/call  {cnt / iters:6.2f} x  {name}")
    if stats:
        Path(stats).parent.mkdir(parents=True, exist_ok=True)
        with open(stats, "a") as fh:
            fh.write(f"== {trace_dir} ==\n" + "\n".join(lines) + "\n")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", choices=sorted(ARMS), default=None)
    ap.add_argument("--summarize", default=None, help="directory of a --trace run under rocprofv3")
    ap.add_argument("--stats", default=None, help="append the per-kernel table of --summarize to this file")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.iters, a.stats)
    elif a.trace:
        trace(a.trace, a.iters, a.warmup)
    else:
        main(a.iters, a.repeats, a.warmup, a.json)

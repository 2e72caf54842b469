#!/usr/bin/env python3
"""Timings of the 2-D point-mass kernels (csrc/trk_planar.hip) on the MI355X, and of a pure-torch restatement of the reference's
path (primitives.py / grid_map_sdf.py / distance_fields.py as torch ops, on the same GPU) as the baseline.

    python tools/bench_pointmass2d.py [--reps 200] [--json out.json]

Rows: cost + gradient on EnvDense2D (400 x 400 grid) and EnvNarrowPassageDense2D (analytic) at 4096 x 64 and 32768 x 64 samples,
the boolean check, and get_trajs_collision_and_free on 4096 trajectories x 64 x 5 via points.  Times are CUDA-event medians of the
Python call (host overhead included); the kernel time itself comes from a `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

import torch_robotics_amd as tra
from torch_robotics_amd.environments import planar_tables

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


class TorchReference:
    """The reference's cost path as torch ops (what it runs on a GPU): per-object SDF through the primitive fields, the grid's gather
    + surrogate, max over objects, the four workspace faces, autograd for the gradient."""

    def __init__(self, task):
        self.m = float(task.df_collision_objects._margin_vector(1)[0])
        objs = task.env.get_df_obj_list()
        self.grid = objs.pop(0) if isinstance(objs[0], tra.GridMapSDF) else None
        objects, prims = planar_tables(objs)
        self.objs = []
        for pos, R, b, e in objects:
            p = torch.as_tensor(prims[b:e], device=DEV)
            sph, box = p[p[:, 0] == 0], p[p[:, 0] == 1]
            self.objs.append((sph[:, 1:3], sph[:, 5], box[:, 1:3], box[:, 3:5], box[:, 5]))
        self.ws_min, self.ws_max = task.ws_min.to(DEV), task.ws_max.to(DEV)
        if self.grid is not None:
            g = self.grid
            self.lo, self.md = g.limits[0].to(DEV), g.map_dim.to(DEV)
            self.dims = torch.tensor(g.sdf_tensor.shape, device=DEV)
            self.sdf, self.gsdf = g.sdf_tensor.contiguous(), g.grad_sdf_tensor.contiguous()

    def cost(self, x):
        dfs = []
        if self.grid is not None:
            idx = ((x - self.lo) / self.md * self.dims).floor().to(torch.int).clamp(torch.zeros_like(self.dims), self.dims - 1).detach()
            i, j = idx.unbind(-1)
            g = self.gsdf[i, j]
            dfs.append(self.sdf[i, j] + (x * g).sum(-1) - (x.detach() * g).sum(-1))
        for c, r, bc, bh, br in self.objs:
            parts = []
            if len(c):
                parts.append(torch.min(torch.norm(x.unsqueeze(-2) - c, dim=-1) - r, dim=-1)[0])
            if len(bc):
                qq = torch.abs(x.unsqueeze(-2) - bc) - bh + br.unsqueeze(-1)
                mq = torch.amax(qq, dim=-1)
                parts.append(torch.min(torch.minimum(mq, torch.zeros_like(mq)) + torch.linalg.norm(torch.relu(qq), dim=-1) - br, dim=-1)[0])
            dfs.append(torch.min(torch.stack(parts, -1), -1)[0])
        obj = torch.relu(self.m - torch.stack(dfs, -2)).max(-2)[0]
        dmin, dmax = x - self.ws_min, self.ws_max - x
        ws = torch.relu(self.m - torch.cat([torch.sign(dmin) * torch.abs(dmin), torch.sign(dmax) * torch.abs(dmax)], -1)).max(-1)[0]
        return obj + ws

    def cost_grad(self, q):
        x = q.detach().requires_grad_(True)
        c = self.cost(x)
        c.sum().backward()
        return c, x.grad


def main(reps=200, out=None):
    rows = []
    for name in ("EnvDense2D", "EnvNarrowPassageDense2D"):
        task = tra.PlanningTask(env=getattr(tra, name)(tensor_args=TA), robot=tra.RobotPointMass(tensor_args=TA), clamp_sdf=True,
                                tensor_args=TA)
        ref = TorchReference(task)
        for B in (4096, 32768):
            q = ((torch.rand(B, 64, 2, device=DEV) - 0.5) * 2.0).requires_grad_(True)

            def ours():
                task.compute_collision_cost(q).sum().backward()
            t_ours = timed(ours, reps)
            t_ref = timed(lambda: ref.cost_grad(q), max(20, reps // 4))
            c_ref, g_ref = ref.cost_grad(q)
            q.grad = None
            c = task.compute_collision_cost(q)
            c.sum().backward()
            err = float((c - c_ref).abs().max())
            t_bool = timed(lambda: task.compute_collision(q.detach()), reps)
            rows.append(dict(scene=name, samples=f"{B} x 64", cost_grad_us=round(t_ours, 2), torch_reference_us=round(t_ref, 1),
                             speedup=round(t_ref / t_ours, 1), collision_us=round(t_bool, 2), max_abs_cost_diff=err,
                             bytes_per_launch=B * 64 * 20))
            print(json.dumps(rows[-1]), flush=True)
        trajs = torch.cat([(torch.rand(4096, 64, 2, device=DEV) - 0.5) * 1.9, torch.zeros(4096, 64, 2, device=DEV)], -1)
        t_val = timed(lambda: task.get_trajs_collision_and_free(trajs, return_indices=True), max(20, reps // 4))
        rows.append(dict(scene=name, validation="4096 trajectories x 64 x 5 via points", get_trajs_collision_and_free_us=round(t_val, 1)))
        print(json.dumps(rows[-1]), flush=True)
    if out:
        Path(out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    main(a.reps, a.json)

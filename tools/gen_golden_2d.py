"""Fixtures of the 2-D point-mass path, recorded from the reference on the CPU.

TEST INFRASTRUCTURE -- never imported by the product, and run only where the reference checkout exists.  It imports the reference
read-only (with the stand-in parser of oracle/refshim on the path) and writes

  tests/golden/scenes_2d.npz          per scene: limits, default grid cell size, whether the grid is on by default, and per object
                                      its pose (3-D pos, wxyz quaternion), fixed / extra, and its primitive fields as tables
  tests/golden/pointmass2d_<S>.npz    seeded inputs and the reference's fp32 outputs for RobotPointMass + PlanningTask on scene S:
                                      cost and gradient (plain and clamp_sdf), booleans at margin 0 and the default margin, the grid
                                      SDF / gradient at sampled cells, compute_sdf and its gradient, edge points, and the index lists
                                      and metrics of get_trajs_collision_and_free (3-D and 4-D batches)

    python tools/gen_golden_2d.py [reference checkout, default /root/reference]
"""
import contextlib
import io
import os
import sys
from pathlib import Path

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
sys.path.insert(0, str(REPO / "oracle" / "refshim"))
sys.path.insert(0, str(REF))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLD = REPO / "tests" / "golden"
TA = dict(device="cpu", dtype=torch.float32)

# scene class -> (module, default grid cell size or None when the scene has no precompute_sdf_obj_fixed default)
SCENES = {
    "EnvSimple2D": "env_simple_2d", "EnvDense2D": "env_dense_2d", "EnvNarrowPassageDense2D": "env_narrow_passage_dense_2d",
    "EnvSquare2D": "env_square_2d", "EnvCircle2D": "env_circle_2d", "EnvGridCircles2D": "env_grid_circles_2d",
    "EnvSimple2DExtraObjects": "env_simple_2d_extra_objects", "EnvDense2DExtraObjects": "env_dense_2d_extra_objects",
    "EnvNarrowPassageDense2DExtraObjects": "env_narrow_passage_dense_2d_extra_objects",
}
KIND = {"MultiSphereField": 0, "MultiBoxField": 1, "MultiRoundedBoxField": 1, "MultiSharpBoxField": 2}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def scene_class(name):
    import importlib
    return getattr(importlib.import_module(f"torch_robotics.environments.{SCENES[name]}"), name)


def default_grid(cls):
    """(grid on by default, default cell size) from the constructor's signature and EnvBase's."""
    import inspect
    from torch_robotics.environments.env_base import EnvBase
    p, base = inspect.signature(cls.__init__).parameters, inspect.signature(EnvBase.__init__).parameters
    on = p["precompute_sdf_obj_fixed"].default if "precompute_sdf_obj_fixed" in p else base["precompute_sdf_obj_fixed"].default
    cell = p["sdf_cell_size"].default if "sdf_cell_size" in p else base["sdf_cell_size"].default
    for c in cls.__mro__[1:]:                     # a subclass that forwards **kwargs inherits its parent's defaults
        if c is EnvBase or "precompute_sdf_obj_fixed" in p:
            break
        pc = inspect.signature(c.__init__).parameters
        if "precompute_sdf_obj_fixed" in pc:
            on, cell = pc["precompute_sdf_obj_fixed"].default, pc["sdf_cell_size"].default
            break
    return bool(on), float(cell)


def scene_tables(name, env, on, cell):
    """Flat arrays of one scene.  Field rows: [object, field, kind, n_rows]; primitive rows: [cx, cy, a, b] with (a, b) = (radius, 0)
    for spheres and the two sizes for boxes, in the field's order."""
    objs = [(o, 0) for o in (env.obj_fixed_list or [])] + [(o, 1) for o in (env.obj_extra_list or [])]
    pos, ori, extra, names, fields, prims = [], [], [], [], [], []
    for k, (o, ex) in enumerate(objs):
        pos.append(o.pos.numpy().reshape(3)); ori.append(o.ori.numpy().reshape(4)); extra.append(ex); names.append(o.name)
        for j, f in enumerate(o.fields):
            kind = KIND[type(f).__name__]
            c = f.centers.numpy().reshape(-1, 2)
            ab = np.stack([f.radii.numpy().reshape(-1), np.zeros(len(c), np.float32)], 1) if kind == 0 else f.sizes.numpy().reshape(-1, 2)
            fields.append([k, j, kind, len(c)])
            prims.append(np.concatenate([c, ab], 1))
    return {f"{name}/limits": env.limits.numpy(), f"{name}/grid_on": np.bool_(on), f"{name}/cell": np.float32(cell),
            f"{name}/obj_pos": np.array(pos, np.float32), f"{name}/obj_ori": np.array(ori, np.float32),
            f"{name}/obj_extra": np.array(extra, np.int32), f"{name}/obj_name": np.array(names),
            f"{name}/fields": np.array(fields, np.int32), f"{name}/prims": np.concatenate(prims, 0).astype(np.float32)}


def edge_points(env_limits, cell):
    """Points on the workspace faces and corners, outside the limits, on grid-cell boundaries and with -0.0 coordinates."""
    lo, hi = env_limits[0].numpy().astype(np.float32), env_limits[1].numpy().astype(np.float32)
    pts = [[lo[0], 0.3], [hi[0], -0.2], [0.1, lo[1]], [-0.4, hi[1]], [lo[0], lo[1]], [hi[0], hi[1]],
           [-1.3, 0.2], [0.5, 1.7], [2.0, -2.0], [-0.0, -0.0], [-0.0, 0.55], [0.35, -0.0], [0.0, 0.0]]
    n = np.float32(round(2.0 / cell))
    for i in (1, 37, 200, 311):                  # exact multiples of the cell size off lim_min
        pts.append([np.float32(lo[0] + np.float32(i) * np.float32(2.0) / n), np.float32(-0.45)])
        pts.append([np.float32(0.62), np.float32(lo[1] + np.float32(i) * np.float32(2.0) / n)])
    return np.array(pts, np.float32)


def scene_goldens(name, cls, on, cell, seed):
    from torch_robotics.robots.robot_point_mass import RobotPointMass
    from torch_robotics.tasks.tasks import PlanningTask
    env = quiet(cls, tensor_args=TA)
    robot = quiet(RobotPointMass, tensor_args=TA)
    task = PlanningTask(env=env, robot=robot, tensor_args=TA)
    gen = torch.Generator().manual_seed(seed)
    q = ((torch.rand(16, 32, 2, generator=gen) - 0.5) * 2.3)                 # a few points outside the workspace
    q_edge = torch.from_numpy(edge_points(env.limits, cell))
    out = dict(q=q.numpy(), q_edge=q_edge.numpy(), cutoff=np.float32(task.df_collision_objects.cutoff_margin),
               margins=robot.link_margins_for_object_collision_checking_tensor.numpy(), q_limits=robot.q_limits.numpy())
    for tag, clamp in (("", False), ("_c", True)):
        for fld in (task.df_collision_objects, task.df_collision_ws_boundaries):
            fld.clamp_sdf = clamp
        for qq, suf in ((q, ""), (q_edge, "_edge")):
            x = qq.clone().requires_grad_(True)
            cost = task.compute_collision_cost(x)
            (g,) = torch.autograd.grad(cost.sum(), x)
            out[f"cost{tag}{suf}"], out[f"gq{tag}{suf}"] = cost.detach().numpy(), g.numpy()
    for qq, suf in ((q, ""), (q_edge, "_edge")):
        out[f"coll{suf}"] = task.compute_collision(qq).numpy()
        out[f"coll0{suf}"] = task.compute_collision(qq, margin=0.0).numpy()
        x = qq.clone().requires_grad_(True)
        sdf = env.compute_sdf(x)
        (gs,) = torch.autograd.grad(sdf.sum(), x)
        out[f"sdf{suf}"], out[f"gsdf{suf}"] = sdf.detach().numpy(), gs.numpy()
    gm = env.grid_map_sdf_obj_fixed
    if gm is not None:
        dims = np.array(gm.sdf_tensor.shape, np.int64)
        rng = np.random.default_rng(seed)
        cells = np.concatenate([rng.integers(0, dims, size=(3000, 2)), [[0, 0], dims - 1, [0, dims[1] - 1], [dims[0] - 1, 0]]])
        out.update(grid_dims=dims, grid_cells=cells.astype(np.int32),
                   grid_sdf=gm.sdf_tensor[cells[:, 0], cells[:, 1]].numpy(), grid_grad=gm.grad_sdf_tensor[cells[:, 0], cells[:, 1]].numpy())
    # trajectories: straight lines between random points plus noise, velocities carried in the state; some leave the limits
    T, H = 48, 16
    a, b = (torch.rand(T, 2, generator=gen) - 0.5) * 1.9, (torch.rand(T, 2, generator=gen) - 0.5) * 1.9
    s = torch.linspace(0, 1, H).view(1, H, 1)
    pos = a.view(T, 1, 2) * (1 - s) + b.view(T, 1, 2) * s + 0.01 * torch.randn(T, H, 2, generator=gen)
    pos[-3:] *= 1.2                                                             # the last three reach past the joint limits
    trajs = torch.cat([pos, torch.randn(T, H, 2, generator=gen) * 0.1], -1)
    out["trajs"] = trajs.numpy()
    for suf, tr in (("", trajs), ("_4d", trajs.reshape(4, 12, H, 4))):
        try:
            tc, ci, tf, fi, wp = task.get_trajs_collision_and_free(tr, return_indices=True)
        except IndexError:          # the reference's 4-D branch indexes a 1-D row when exactly one trajectory is free (tasks.py:285)
            assert suf == "_4d"
            continue
        out[f"coll_idxs{suf}"], out[f"free_idxs{suf}"], out[f"wp{suf}"] = ci.numpy(), fi.numpy(), wp.numpy()
        out[f"fraction_free{suf}"] = np.float64(task.compute_fraction_free_trajs(tr))
        out[f"intensity{suf}"] = np.float64(task.compute_collision_intensity_trajs(tr))
        out[f"success{suf}"] = np.int32(task.compute_success_free_trajs(tr))
    np.savez_compressed(GOLD / f"pointmass2d_{name}.npz", **out)
    print(f"pointmass2d_{name}: free {len(out['free_idxs'])} / {T}, grid {gm is not None}")


def main():
    tables = {}
    for k, name in enumerate(SCENES):
        cls = scene_class(name)
        on, cell = default_grid(cls)
        env = quiet(cls, tensor_args=TA, precompute_sdf_obj_fixed=False)
        tables.update(scene_tables(name, env, on, cell))
        scene_goldens(name, cls, on, cell, seed=2000 + k)
    np.savez_compressed(GOLD / "scenes_2d.npz", **tables)
    print("scenes_2d:", len(SCENES), "scenes")


if __name__ == "__main__":
    main()

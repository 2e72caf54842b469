"""Fixtures of the 2-D point-mass path, recorded from the reference on the CPU.

TEST INFRASTRUCTURE -- never imported by the product, and run only where the reference checkout exists.  It imports the reference
read-only (with the stand-in parser of oracle/refshim on the path) and writes

  tests/golden/scenes_2d.npz          per scene: limits, default grid cell size, whether the grid is on by default, and per object
                                      its pose (3-D pos, wxyz quaternion), fixed / extra, and its primitive fields as tables
  tests/golden/pointmass2d_<S>.npz    seeded inputs and the reference's fp32 outputs for RobotPointMass + PlanningTask on scene S:
                                      cost and gradient (plain and clamp_sdf), booleans at margin 0 and the default margin, the grid
                                      SDF / gradient at sampled cells, compute_sdf and its gradient, edge points, and the index lists
                                      and metrics of get_trajs_collision_and_free (3-D and 4-D batches)

  tests/golden/pointmass2d_synth_<S>.npz   the same outputs for SYNTHETIC scenes built here from the reference's own classes (posed
                                      objects, sharp boxes, non-square grids, exact ties), each file carrying its scene as data under
                                      'scene/...' in scene_tables' layout, per-object distances, the grid's tie nodes, and the largest
                                      deviation of the reference's fp32 distances from the fp64 restatement of tests/helpers.py over
                                      the seeded batch the GPU tests use ('band_measured')

A file is rewritten only when its arrays differ from what is on disk, and archives are written with a fixed time stamp, so a second
run leaves every file byte-identical.  The nine older fixtures and scenes_2d.npz were written by np.savez_compressed: they keep their
bytes because their arrays are unchanged; one whose arrays did change would be rewritten through the fixed-stamp writer.

    python tools/gen_golden_2d.py [reference checkout]
"""
import contextlib
import io
import os
import sys
from pathlib import Path

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(sys.argv[1] if len(sys.argv) > 1 else REPO.parent / "reference")
sys.path.insert(0, str(REPO / "oracle" / "refshim"))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO))

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


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp; the file is left alone when it already holds exactly these arrays."""
    import zipfile
    arrays = {k: np.asanyarray(v) for k, v in arrays.items()}
    if path.exists():
        with np.load(path) as z:
            if list(z.files) == list(arrays) and all(z[k].dtype == v.dtype and z[k].shape == v.shape and
                                                       np.array_equal(z[k], v, equal_nan=v.dtype.kind == "f") and
                                                       (v.dtype.kind != "f" or np.array_equal(np.signbit(z[k]), np.signbit(v)))
                                                       for k, v in arrays.items()):
                return False
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, v, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    return True


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
    out = record(env, robot, task, q, q_edge, seed)
    # trajectories: straight lines between random points plus noise, velocities carried in the state; some leave the limits
    T, H = 48, 16
    a, b = (torch.rand(T, 2, generator=gen) - 0.5) * 1.9, (torch.rand(T, 2, generator=gen) - 0.5) * 1.9
    record_trajs(task, out, a, b, gen, T, H)
    wrote = save_npz(GOLD / f"pointmass2d_{name}.npz", out)
    print(f"pointmass2d_{name}: free {len(out['free_idxs'])} / {T}, grid {env.grid_map_sdf_obj_fixed is not None}, "
          f"{'written' if wrote else 'unchanged'}")


def record(env, robot, task, q, q_edge, seed, n_cells=3000):
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
    for fld in (task.df_collision_objects, task.df_collision_ws_boundaries):
        fld.clamp_sdf = False
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
        cells = np.concatenate([rng.integers(0, dims, size=(n_cells, 2)), [[0, 0], dims - 1, [0, dims[1] - 1], [dims[0] - 1, 0]]])
        out.update(grid_dims=dims, grid_cells=cells.astype(np.int32),
                   grid_sdf=gm.sdf_tensor[cells[:, 0], cells[:, 1]].numpy(), grid_grad=gm.grad_sdf_tensor[cells[:, 0], cells[:, 1]].numpy())
    return out


def record_trajs(task, out, a, b, gen, T, H):
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


# ---------------------------------------------------------------------------------------------------------------------------
# synthetic scenes: what the nine recorded scenes never exercise (object poses, sharp boxes, non-square grids, exact ties)
# ---------------------------------------------------------------------------------------------------------------------------
SYNTH = ["ties", "posed", "sharp", "gridposed", "gridtie", "gridthin"]
LIM = [[-1.0, -0.6], [1.0, 0.9]]                 # non-square and off-centre: nx != ny, lim0 != lim1, md0 != md1
F32 = np.float32


def rot_z(deg):
    return [np.cos(np.deg2rad(deg) / 2), 0.0, 0.0, np.sin(np.deg2rad(deg) / 2)]


def exact_round_box_size():
    """A box size s (a multiple of 1/256) whose rounding radius r = fl(0.15 s) makes h - r exact in fp32 for h = s / 2, so that the point
    |dx| = h - r has max_q == 0 exactly."""
    for k in range(40, 160):
        s = F32(k) / F32(256)
        h, r = s / F32(2), s * F32(0.15)
        x = F32(h - r)
        if np.float64(x) == np.float64(h) - np.float64(r) and F32(F32(x - h) + r) == 0:
            return float(s)
    raise AssertionError("no exact size")


def synth_objects(name):
    """[(fields [(class name, centers, sizes or radii)], object name, pos, ori wxyz, extra)], limits, cell size, grid on"""
    S, B, X = "MultiSphereField", "MultiBoxField", "MultiSharpBoxField"
    s0 = exact_round_box_size()
    if name == "ties":                           # identity and power-of-two translated poses: every tie below is exact in fp32
        return [([(S, [[-0.5, 0.25], [-0.5, -0.25], [0.0, 0.5]], [0.125, 0.125, 1 / 64])], "spheres", None, None, 0),
                ([(X, [[0.0, 0.0]], [[0.25, 0.25]])], "sharp-origin", None, None, 0),
                ([(B, [[0.0, 0.0]], [[2 * s0, s0]])], "round-origin", None, None, 0),
                ([(S, [[0.0, 0.5]], [0.125]), (X, [[0.0, 0.0]], [[0.25, 0.25]]), (B, [[0.0, -0.5]], [[0.25, 0.125]])],
                 "three-kinds", [0.5, 0.25, 0.0], [1.0, 0.0, 0.0, 0.0], 0),
                ([(S, [[-0.5, 0.75]], [0.125])], "far-sphere", None, None, 0)], LIM, 0.013, False
    if name == "posed":
        return [([(B, [[0.0, 0.0], [0.1, 0.3]], [[0.2, 0.3], [0.15, 0.1]])], "translated", [0.3, -0.2, 0.0], [1.0, 0.0, 0.0, 0.0], 0),
                ([(S, [[0.05, 0.1], [-0.2, 0.0]], [0.1, 0.07]), (X, [[0.0, -0.15]], [[0.3, 0.1]]), (B, [[0.2, 0.15]], [[0.12, 0.2]])],
                 "rot-z", [-0.45, 0.35, 0.0], rot_z(33.0), 0),
                ([(B, [[0.0, 0.0]], [[0.4, 0.25]]), (S, [[0.25, 0.2]], [0.08])], "tilted", [-0.4, -0.3, 0.15],
                 [1.7, 0.5, -0.3, 0.9], 0)], LIM, 0.013, False          # tilt about x and y, pos[2] != 0, |ori| != 1
    if name == "sharp":
        return [([(X, [[0.4, 0.3], [-0.3, -0.2], [0.5, -0.35]], [[0.3, 0.2], [0.2, 0.4], [0.15, 0.15]])], "sharp", None, None, 0),
                ([(X, [[0.0, 0.0], [0.25, 0.1]], [[0.2, 0.1], [0.1, 0.3]])], "sharp-rot", [-0.5, 0.45, 0.0], rot_z(-20.0), 0)], LIM, 0.013, False
    if name == "gridposed":                      # posed fixed objects in the grid, analytic extra objects after it; 154 x 116 cells
        return [([(S, [[0.05, 0.1]], [0.12]), (X, [[0.0, -0.15]], [[0.3, 0.1]])], "rot-z", [-0.45, 0.35, 0.0], rot_z(33.0), 0),
                ([(B, [[0.0, 0.0]], [[0.4, 0.25]])], "tilted", [0.45, 0.4, 0.15], [1.7, 0.5, -0.3, 0.9], 0),
                ([(X, [[0.0, 0.0]], [[0.2, 0.3]]), (S, [[0.3, 0.1]], [0.1])], "extra", [0.25, -0.25, 0.0], [1.0, 0.0, 0.0, 0.0], 1),
                ([(B, [[0.0, 0.0]], [[0.25, 0.15]])], "extra-rot", [-0.5, -0.3, 0.0], rot_z(50.0), 1)], LIM, 0.013, True
    if name == "gridtie":                        # 65 x 49 nodes, all multiples of 1/32: the nodes x == 0 are equidistant from the two objects
        return [([(S, [[-0.5, 0.25]], [0.25])], "left", None, None, 0),
                ([(S, [[0.0, 0.0]], [0.25])], "right", [0.5, 0.25, 0.0], [1.0, 0.0, 0.0, 0.0], 0)], [[-1.0, -0.5], [1.0, 1.0]], 0.031, True
    if name == "gridthin":                       # an axis of 3 cells
        return [([(S, [[0.0, 0.0]], [0.2]), (X, [[0.5, 0.0]], [[0.2, 0.04]])], "thin", [-0.3, 0.01, 0.0], [1.0, 0.0, 0.0, 0.0], 0)], \
            [[-1.0, -0.05], [1.0, 0.0625]], 0.05, True
    raise KeyError(name)


def synth_env(name):
    import torch_robotics.environments.primitives as P
    from torch_robotics.environments.env_base import EnvBase
    spec, limits, cell, on = synth_objects(name)
    fixed, extra = [], []
    for fields, oname, pos, ori, ex in spec:
        fl = [getattr(P, c)(np.array(ctr, np.float32), np.array(ab, np.float32), tensor_args=TA) for c, ctr, ab in fields]
        kw = {} if pos is None else dict(pos=torch.tensor(pos, **TA), ori=torch.tensor(ori, **TA))
        (extra if ex else fixed).append(P.ObjectField(fl, oname, **kw))
    make = lambda grid: quiet(EnvBase, name=f"synth_{name}", limits=torch.tensor(limits, **TA), obj_fixed_list=fixed,   # noqa: E731
                              obj_extra_list=extra or None, precompute_sdf_obj_fixed=grid, sdf_cell_size=cell, tensor_args=TA)
    return make, on, cell


def synth_edge_points(name, env, margin):
    """The recorded edge points: workspace faces and corners of the non-square box, outside points, cell boundaries of the non-square
    grid, and for 'ties' the exact ties and kinks of the kernel header's rules."""
    lo, hi = env.limits[0].numpy().astype(F32), env.limits[1].numpy().astype(F32)
    my = F32(0.5) * (lo[1] + hi[1])
    pts = [[lo[0], my], [hi[0], my], [0.125, lo[1]], [-0.375, hi[1]], [lo[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]], [hi[0], lo[1]],
           [-1.3, 0.2], [0.5, 1.7], [2.0, -2.0], [-0.0, -0.0], [0.0, 0.0], [-0.0, 0.0]]
    gm = env.grid_map_sdf_obj_fixed
    if gm is not None:
        nx, ny = (F32(v) for v in gm.sdf_tensor.shape)
        for i in (1, 2, 37):                     # exact multiples of the cell pitch off lim_min, per axis
            pts.append([F32(lo[0] + F32(i) * (hi[0] - lo[0]) / nx), my])
            pts.append([F32(0.3), F32(lo[1] + F32(min(i, int(ny) - 1)) * (hi[1] - lo[1]) / ny)])
    if name == "ties":
        s0 = F32(exact_round_box_size())
        h, r = s0 / F32(2), s0 * F32(0.15)
        xh = F32(F32(1 / 64) + margin)
        assert F32(xh - F32(1 / 64)) == margin and F32(F32(h - r) - h) + r == 0
        pts += [[-0.5, 0.25], [0.5, 0.75],                       # centres of spheres (identity and translated object)
                [0.5, 0.25], [0.5, -0.25],                       # centres of the translated sharp and rounded boxes
                [0.0625, 0.0625], [-0.0625, 0.0625],             # diagonal of the sharp box at the origin
                [F32(0.25) * s0, 0.0],                           # inside the rounded box at the origin, off the diagonal
                [F32(s0 - F32(0.25) * s0), F32(0.25) * s0],     # ux == uy inside the rounded box (2 s0 x s0): |dx| - s0 == |dy| - s0 / 2
                [F32(s0 - r), 0.0], [0.0, F32(h - r)], [F32(s0 - r), F32(h - r)],     # max_q == 0 on x, on y, on both
                [0.75, 0.5], [0.625, 0.375],                     # diagonals of the translated sharp box, outside and on its corner
                [-0.5, 0.0],                                     # equidistant from two spheres of one field
                [0.5, 0.5],                                      # equidistant from the sphere field and the sharp-box field of one object
                [-0.5, 0.5],                                     # equidistant from two objects
                [xh, 0.5], [-xh, 0.5]]                           # the hinge margin - sdf is exactly 0 (sphere of radius 1/64)
    return np.array(pts, F32)


def synth_goldens(name, seed):
    import helpers
    from torch_robotics.robots.robot_point_mass import RobotPointMass
    from torch_robotics.tasks.tasks import PlanningTask
    make, on, cell = synth_env(name)
    env = make(on)
    robot = quiet(RobotPointMass, tensor_args=TA)
    task = PlanningTask(env=env, robot=robot, tensor_args=TA)
    margin = F32(F32(robot.link_margins_for_object_collision_checking_tensor.numpy()[0]) + F32(task.df_collision_objects.cutoff_margin))
    gen = torch.Generator().manual_seed(seed)
    lo, hi = env.limits[0], env.limits[1]
    q = lo + (hi - lo) * (0.5 + (torch.rand(16, 32, 2, generator=gen) - 0.5) * 1.15)
    q_edge = torch.from_numpy(synth_edge_points(name, env, margin))
    out = {f"scene/{k.split('/', 1)[1]}": v for k, v in scene_tables(name, make(False), on, cell).items()}
    out.update(record(env, robot, task, q, q_edge, seed, n_cells=2000))
    objs = list(env.obj_fixed_list or []) + list(env.obj_extra_list or [])
    for qq, suf in ((q.reshape(-1, 2), ""), (q_edge, "_edge")):          # every object on its own: ObjectField.compute_signed_distance
        x = qq.clone().requires_grad_(True)
        per = torch.stack([o.compute_signed_distance(x) for o in objs], -1)
        out[f"obj_sdf{suf}"] = per.detach().numpy()
        out[f"obj_gsdf{suf}"] = np.stack([torch.autograd.grad(per[:, k].sum(), x, retain_graph=True)[0].numpy() for k in range(len(objs))], 1)
    gm = env.grid_map_sdf_obj_fixed
    if gm is not None:                           # the nodes where two fixed objects are exactly equidistant: torch.minimum shares the gradient
        pts = gm.points_for_sdf.reshape(-1, 2)
        per = torch.stack([o.compute_signed_distance(pts) for o in env.obj_fixed_list], -1)
        srt = per.sort(-1).values
        tie = (srt[:, 0] == srt[:, 1]).reshape(gm.sdf_tensor.shape) if per.shape[1] > 1 else torch.zeros(gm.sdf_tensor.shape, dtype=torch.bool)
        cells = tie.nonzero().numpy().astype(np.int32)
        out.update(grid_tie_cells=cells, grid_tie_sdf=gm.sdf_tensor[cells[:, 0], cells[:, 1]].numpy(),
                   grid_tie_grad=gm.grad_sdf_tensor[cells[:, 0], cells[:, 1]].numpy())
    T, H = 48, 16
    a, b = (lo + (hi - lo) * (0.5 + (torch.rand(T, 2, generator=gen) - 0.5) * 0.95) for _ in range(2))
    record_trajs(task, out, a, b, gen, T, H)

    # the reference's own fp32 distances against the fp64 restatement over the batch the GPU tests use: the boolean band
    scene = helpers.planar_fixture_scene(out)
    ladder_objs = [o for o in scene["objects"] if o["extra"] or gm is None]
    qb = helpers.planar_batch(ladder_objs, scene["limits"], helpers.planar_margins(margin), helpers.PLANAR_BATCH_N, seed)
    grid = None if gm is None else dict(sdf=gm.sdf_tensor.numpy(), grad=gm.grad_sdf_tensor.numpy(), lo=gm.limits[0].numpy(), md=gm.map_dim.numpy())
    ws = (scene["limits"][0], scene["limits"][1])
    xb = torch.from_numpy(qb)
    dev, bad = 0.0, 0
    for clamp in (False, True):
        c64, g64, s64, _ = helpers.planar64(ladder_objs, qb, margin, ws=ws, grid=grid, clamp=clamp)
        s32 = torch.stack([d.compute_signed_distance(xb) for d in env.get_df_obj_list()], -1).numpy()
        f32 = torch.cat([xb - env.limits[0], env.limits[1] - xb], -1).numpy()
        f64 = np.concatenate([qb.astype(np.float64) - scene["limits"][0], scene["limits"][1].astype(np.float64) - qb], -1)
        dev = max(dev, float(np.abs(s32 - s64).max()), float(np.abs(f32 - f64).max()))
        for fld in (task.df_collision_objects, task.df_collision_ws_boundaries):
            fld.clamp_sdf = clamp
        x = xb.clone().requires_grad_(True)
        c32 = task.compute_collision_cost(x)
        (g32,) = torch.autograd.grad(c32.sum(), x)
        assert helpers.rel_err(c32.detach().numpy().reshape(-1), c64) < 1e-5, (name, clamp)
        rows = helpers.planar_bad_rows(g32.numpy(), g64)
        if clamp:                                # within the band of a hinge fp32 and fp64 may sit on either side of relu's kink: such a
            und = ~helpers.planar_hinge_decided(s64, qb, ws, float(margin), 2 * dev)   # row must carry one of the one-sided fp64 gradients
            sides = helpers.planar_hinge_sides64(ladder_objs, qb[und], float(margin), 4 * dev, ws=ws, grid=grid)
            assert helpers.planar_rows_match_any(g32.numpy()[und], sides).all(), (name, "hinge rows")
            rows &= ~und
        bad = max(bad, int(rows.sum()))
    d64 = np.minimum(s64.min(-1), f64.min(-1))
    counts = [[int(((d64 - mm > 2 * dev) & (d64 - mm <= 20 * dev)).sum()), int(((mm - d64 > 2 * dev) & (mm - d64 <= 20 * dev)).sum())]
              for mm in helpers.planar_margins(margin)]
    print("   decided samples within ten bands (above, below) per margin:", counts)
    assert bad <= len(qb) // 10000, (name, bad)    # the reference's own fp32 run stays within the kink share on this seed
    out["band_measured"] = np.float64(dev)
    out["batch_seed"] = np.int64(seed)
    path = GOLD / f"pointmass2d_synth_{name}.npz"
    wrote = save_npz(path, out)
    print(f"pointmass2d_synth_{name}: free {len(out['free_idxs'])} / {T}, grid {None if gm is None else tuple(gm.sdf_tensor.shape)}, "
          f"tie nodes {len(out['grid_tie_cells']) if gm is not None else '-'}, band {dev:.3e}, kink rows {bad}, {path.stat().st_size} bytes, "
          f"{'written' if wrote else 'unchanged'}")


def main():
    tables = {}
    for k, name in enumerate(SCENES):
        cls = scene_class(name)
        on, cell = default_grid(cls)
        env = quiet(cls, tensor_args=TA, precompute_sdf_obj_fixed=False)
        tables.update(scene_tables(name, env, on, cell))
        scene_goldens(name, cls, on, cell, seed=2000 + k)
    wrote = save_npz(GOLD / "scenes_2d.npz", tables)
    print("scenes_2d:", len(SCENES), "scenes,", "written" if wrote else "unchanged")
    for k, name in enumerate(SYNTH):
        synth_goldens(name, seed=3000 + k)


if __name__ == "__main__":
    main()

"""The 2-D point mass on the MI355X: RobotPointMass + PlanningTask on every 2-D scene against the reference's recorded outputs
(tests/golden/pointmass2d_*.npz, tools/gen_golden_2d.py), a full-size batch against an fp64 torch restatement, and the edges."""
import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
from helpers import gold, grad_close, rel_err
from torch_robotics_amd import ops
from torch_robotics_amd.environments import planar_tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
TOL_C = 1e-5
NAMES = ["EnvSimple2D", "EnvDense2D", "EnvNarrowPassageDense2D", "EnvSquare2D", "EnvCircle2D", "EnvGridCircles2D",
         "EnvSimple2DExtraObjects", "EnvDense2DExtraObjects", "EnvNarrowPassageDense2DExtraObjects"]
_tasks = {}


def task_of(name):
    if name not in _tasks:
        env = getattr(tra, name)(tensor_args=TA)
        _tasks[name] = tra.PlanningTask(env=env, robot=tra.RobotPointMass(tensor_args=TA), tensor_args=TA)
    return _tasks[name]


def set_clamp(task, on):
    for f in (task.df_collision_objects, task.df_collision_ws_boundaries):
        f.clamp_sdf = on


def dev(a):
    return torch.as_tensor(np.asarray(a), device=DEV)


@pytest.mark.parametrize("name", NAMES)
def test_cost_and_gradient_like_the_reference(name):
    g, task = gold(f"pointmass2d_{name}"), task_of(name)
    np.testing.assert_array_equal(task.robot.q_limits.cpu().numpy(), g["q_limits"])
    for tag, clamp in (("", False), ("_c", True)):
        set_clamp(task, clamp)
        try:
            for suf in ("", "_edge"):
                q = dev(g[f"q{suf}"]).requires_grad_(True)
                cost = task.compute_collision_cost(q)
                assert cost.shape == g[f"cost{tag}{suf}"].shape
                assert rel_err(cost.detach().cpu().numpy(), g[f"cost{tag}{suf}"]) < TOL_C, (tag, suf)
                cost.sum().backward()
                assert grad_close(q.grad.cpu().numpy(), g[f"gq{tag}{suf}"]), (tag, suf)
                with torch.no_grad():                                     # the launch without the gradient output agrees
                    np.testing.assert_array_equal(task.compute_collision_cost(q).cpu().numpy(), cost.detach().cpu().numpy())
        finally:
            set_clamp(task, False)


@pytest.mark.parametrize("name", NAMES)
def test_booleans_at_both_margins(name):
    g, task = gold(f"pointmass2d_{name}"), task_of(name)
    for suf in ("", "_edge"):
        q = dev(g[f"q{suf}"])
        np.testing.assert_array_equal(task.compute_collision(q).cpu().numpy(), g[f"coll{suf}"])
        np.testing.assert_array_equal(task.compute_collision(q, margin=0.0).cpu().numpy(), g[f"coll0{suf}"])


@pytest.mark.parametrize("name", [n for n in NAMES if "grid_dims" in gold(f"pointmass2d_{n}").files])
def test_grid_at_sampled_cells(name):
    g, task = gold(f"pointmass2d_{name}"), task_of(name)
    gm = task.env.grid_map_sdf_obj_fixed
    assert tuple(gm.sdf_tensor.shape) == tuple(g["grid_dims"]) and tuple(gm.grad_sdf_tensor.shape) == tuple(g["grid_dims"]) + (2,)
    c = g["grid_cells"]
    sdf = gm.sdf_tensor[c[:, 0], c[:, 1]].cpu().numpy()
    grad = gm.grad_sdf_tensor[c[:, 0], c[:, 1]].cpu().numpy()
    assert rel_err(sdf, g["grid_sdf"]) < TOL_C
    assert grad_close(grad, g["grid_grad"])


@pytest.mark.parametrize("name", NAMES)
def test_compute_sdf(name):
    g, task = gold(f"pointmass2d_{name}"), task_of(name)
    for suf in ("", "_edge"):
        x = dev(g[f"q{suf}"]).requires_grad_(True)
        sdf = task.env.compute_sdf(x)
        assert sdf.shape == g[f"sdf{suf}"].shape and rel_err(sdf.detach().cpu().numpy(), g[f"sdf{suf}"]) < TOL_C
        sdf.sum().backward()
        assert grad_close(x.grad.cpu().numpy(), g[f"gsdf{suf}"])


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_validation(name):
    g, task = gold(f"pointmass2d_{name}"), task_of(name)
    trajs = dev(g["trajs"])
    for suf, tr in (("", trajs), ("_4d", trajs.reshape(4, 12, *trajs.shape[1:]))):
        if f"coll_idxs{suf}" not in g.files:           # the reference's own 4-D branch raises on this batch (one free trajectory)
            continue
        tc, ci, tf, fi, wp = task.get_trajs_collision_and_free(tr, return_indices=True)
        np.testing.assert_array_equal(wp.cpu().numpy(), g[f"wp{suf}"])
        np.testing.assert_array_equal(ci.cpu().numpy().reshape(g[f"coll_idxs{suf}"].shape), g[f"coll_idxs{suf}"])
        np.testing.assert_array_equal(fi.cpu().numpy().reshape(g[f"free_idxs{suf}"].shape), g[f"free_idxs{suf}"])
        assert task.compute_fraction_free_trajs(tr) == pytest.approx(float(g[f"fraction_free{suf}"]), abs=1e-12)
        assert float(task.compute_collision_intensity_trajs(tr)) == pytest.approx(float(g[f"intensity{suf}"]), abs=1e-6)
        assert task.compute_success_free_trajs(tr) == int(g[f"success{suf}"])
    # the fused via-point launch equals interpolating first and testing the interpolated points
    wp2 = task.compute_collision(ops.interpolate_traj_via_points(trajs, 5), margin=0.0)
    np.testing.assert_array_equal(task._waypoint_collisions(trajs, 5).cpu().numpy(), wp2.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# full size against fp64
# ---------------------------------------------------------------------------------------------------------------------------
def cost64(task, q, clamp):
    """The reference's 2-D objective restated in torch fp64 (primitives.py, grid_map_sdf.py, distance_fields.py): -> cost, grad."""
    x = q.detach().to(torch.float64).requires_grad_(True)
    m = float(task.df_collision_objects._margin_vector(1)[0])
    dfs = []
    objs = task.env.get_df_obj_list()
    if isinstance(objs[0], tra.GridMapSDF):
        gm = objs.pop(0)
        lo, md, dims = gm.limits[0].to(DEV), gm.map_dim.to(DEV), torch.tensor(gm.sdf_tensor.shape, device=DEV)
        idx = ((q.detach() - lo) / md * dims).floor().to(torch.int64)           # the lookup's own fp32 index arithmetic
        idx = torch.minimum(torch.maximum(idx, torch.zeros_like(idx)), dims - 1)
        s = gm.sdf_tensor[idx[:, 0], idx[:, 1]].double()
        gg = gm.grad_sdf_tensor[idx[:, 0], idx[:, 1]].double()
        dfs.append(s + (x * gg).sum(-1) - (x.detach() * gg).sum(-1))
    objects, prims = planar_tables(objs)
    for pos, R, b, e in objects:
        assert np.array_equal(R, np.eye(3)) and not np.any(pos)
        best = None
        for t, cx, cy, hx, hy, r in prims[b:e].astype(np.float64):
            d = x - torch.tensor([cx, cy], device=DEV, dtype=torch.float64)
            if t == 0:
                v = torch.linalg.norm(d, dim=-1) - r
            else:
                u = d.abs() - torch.tensor([hx, hy], device=DEV, dtype=torch.float64) + r
                mu = torch.amax(u, -1)
                v = torch.minimum(mu, torch.zeros_like(mu)) + torch.linalg.norm(torch.relu(u), dim=-1) - r
            best = v if best is None else torch.where(v < best, v, best)
        dfs.append(best)
    c = torch.stack([m - v for v in dfs], -1)
    c = torch.relu(c) if clamp else c
    wmin, wmax = task.ws_min.to(DEV).double(), task.ws_max.to(DEV).double()
    w = m - torch.cat([x - wmin, wmax - x], -1)
    w = torch.relu(w) if clamp else w
    cost = c.max(-1)[0] + w.max(-1)[0]
    (gq,) = torch.autograd.grad(cost.sum(), x)
    return cost.detach(), gq


@pytest.mark.parametrize("name", ["EnvDense2D", "EnvNarrowPassageDense2D", "EnvGridCircles2D", "EnvDense2DExtraObjects"])
@pytest.mark.parametrize("clamp", [False, True])
def test_full_size_against_fp64(name, clamp):
    task = task_of(name)
    set_clamp(task, clamp)
    try:
        gen = torch.Generator(device=DEV).manual_seed(7)
        q = (torch.rand(4096, 64, 2, device=DEV, generator=gen) - 0.5) * 2.2
        x = q.clone().requires_grad_(True)
        cost = task.compute_collision_cost(x)
        cost.sum().backward()
        c64, g64 = cost64(task, q.reshape(-1, 2), clamp)
        assert rel_err(cost.detach().reshape(-1).cpu().numpy(), c64.cpu().numpy()) < TOL_C
        # a sample within fp32 rounding of a tie between two primitives may take the other branch: a handful at most
        bad = ((x.grad.reshape(-1, 2).double() - g64).abs().max(-1).values > 1e-4 * max(1.0, float(g64.abs().max()))).sum().item()
        assert bad <= 4, bad
        coll = task.compute_collision(q)
        assert coll.shape == (4096, 64)
    finally:
        set_clamp(task, False)


# ---------------------------------------------------------------------------------------------------------------------------
# edges, each against the reference's rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_workspace_face_has_zero_gradient():
    """A point exactly on a face: d = 0 there, d/dd (sign(d) |d|) = 0, so the winning face contributes no gradient."""
    task = task_of("EnvSquare2D")                                       # the box is inside; the faces are clear of it
    q = torch.tensor([[-1.0, 0.8], [1.0, -0.8], [0.8, -1.0], [-0.8, 1.0]], device=DEV, requires_grad=True)
    cost = task.compute_collision_cost(q)
    cost.sum().backward()
    m = float(task.df_collision_objects._margin_vector(1)[0])
    c_obj, g_obj = ops.planar_cost_grad(tra.environments.planar_scene(task.env.get_df_obj_list(), DEV, margin=m), q.detach())
    np.testing.assert_allclose(cost.detach().reshape(-1).cpu().numpy(), c_obj.cpu().numpy() + m, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(q.grad.cpu().numpy(), g_obj.cpu().numpy())      # the face adds 0
    assert task.compute_collision(q, margin=0.0).sum() == 0                        # d = 0 is not < 0


def test_outside_the_limits_takes_the_clamped_cell():
    task = task_of("EnvDense2D")
    gm = task.env.grid_map_sdf_obj_fixed
    nx, ny = gm.sdf_tensor.shape
    q = torch.tensor([[-5.0, -5.0], [5.0, 5.0], [-5.0, 5.0], [1.0, 1.0], [1e30, -1e30]], device=DEV)
    sdf = gm.compute_signed_distance(q).cpu().numpy()
    expect = gm.sdf_tensor[[0, nx - 1, 0, nx - 1, nx - 1], [0, ny - 1, ny - 1, ny - 1, 0]].cpu().numpy()
    np.testing.assert_array_equal(sdf, expect)


def test_grid_cell_boundaries_and_signed_zero():
    """On a cell boundary the lookup takes floor((x - lo) / map_dim * n) in fp32, -0.0 and +0.0 land in the same cell."""
    task = task_of("EnvDense2D")
    gm = task.env.grid_map_sdf_obj_fixed
    n = gm.sdf_tensor.shape[0]
    xs = torch.tensor([-1.0 + k * 2.0 / n for k in (1, 2, 37, 200, 399)], dtype=torch.float32)
    q = torch.stack([xs, torch.full_like(xs, 0.25)], -1).to(DEV)
    q = torch.cat([q, torch.tensor([[-0.0, -0.0], [0.0, 0.0], [-0.0, 0.3]], device=DEV)])
    idx = ((q.cpu() - gm.limits[0]) / gm.map_dim * torch.tensor(gm.sdf_tensor.shape)).floor().to(torch.int64).clamp(0, n - 1)
    np.testing.assert_array_equal(gm.compute_signed_distance(q).cpu().numpy(), gm.sdf_tensor[idx[:, 0], idx[:, 1]].cpu().numpy())
    c = task.compute_collision_cost(q)
    assert c[5] == c[6]


def test_signed_zero_in_a_box_gives_zero_gradient():
    """abs'(-0.0) = abs'(0.0) = 0: at the centre of EnvSquare2D's box the box contributes no gradient; what remains is the workspace
    term, whose four faces tie there (d = 1 each) and whose first face, x - x_min, wins: d cost / dq = (-1, 0)."""
    task = task_of("EnvSquare2D")
    q = torch.tensor([[-0.0, -0.0], [0.0, 0.0], [-0.0, 0.0]], device=DEV, requires_grad=True)
    task.compute_collision_cost(q).sum().backward()
    np.testing.assert_array_equal(q.grad.cpu().numpy(), np.array([[-1.0, 0.0]] * 3, np.float32))


def test_random_coll_free_q():
    task = task_of("EnvDense2D")
    free = task.random_coll_free_q(n_samples=64)
    assert free.shape == (64, 2) and not task.compute_collision(free).any()

"""The 2-D point-mass kernels (csrc/trk_planar.hip) beyond the nine recorded scenes: synthetic scenes recorded from the reference
(tests/golden/pointmass2d_synth_*.npz, tools/gen_golden_2d.py) with posed objects, sharp boxes, non-square grids and exact ties, and
seeded batches of every compiled variant against the fp64 restatement of tests/helpers.py (planar64).

Bounds (DESIGN sections 2 and 6b): cost 1e-5 relative; gradients grad_close at 1e-4 with the per-element bound; a sample whose
gradient misses it must be the fp64 gradient of a point within rounding distance (helpers.kink_rows_ok), at most 1 sample in 10 000;
booleans equal the fp64 decision wherever the fp64 distance is further from the margin than the band = 2 x the largest deviation of the
reference's own fp32 distances from fp64 on the same batch, recorded per scene as `band_measured`; exact ties get exact comparison."""
import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
import helpers as hp
from helpers import gold, grad_close, rel_err
from torch_robotics_amd import ops
from torch_robotics_amd.environments import planar_tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
TOL_C = 1e-5
NAMES = hp.SYNTH_2D
GRID_NAMES = ["gridposed", "gridtie", "gridthin"]
SIZES = (1, 63, 64, 65, 255, 256, 257, hp.PLANAR_BATCH_N)
MIN_DECIDED = 200        # per margin and side, of ~3300 rungs per margin.  Counted on the CPU: 834 at the fewest over the whole scenes
                         # (gen_golden_2d.py prints them), 342 over the variants below (ties, workspace only, override margin)
TIE_ROWS = slice(11, 30)  # 'ties': the +-0 centres, diagonals, max_q == 0 points and equidistant points of synth_edge_points
HINGE_ROWS = slice(30, 32)
_cache = {}


def fixture(name):
    g = gold(f"pointmass2d_synth_{name}")
    return g, hp.planar_fixture_scene(g)


def env_of(name, grid=None):
    key = (name, grid)
    if key not in _cache:
        _cache[key] = hp.planar_build_env(tra, fixture(name)[1], TA, grid=grid)
    return _cache[key]


def task_of(name):
    if ("task", name) not in _cache:
        _cache[("task", name)] = tra.PlanningTask(env=env_of(name), robot=tra.RobotPointMass(tensor_args=TA), tensor_args=TA)
    return _cache[("task", name)]


def set_clamp(task, on):
    for f in (task.df_collision_objects, task.df_collision_ws_boundaries):
        f.clamp_sdf = on


def dev(a):
    return torch.as_tensor(np.asarray(a), device=DEV)


def margin_of(g):
    return np.float32(np.float32(g["margins"][0]) + np.float32(g["cutoff"]))


# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic scenes through the Python API, against their fixtures
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cost_and_gradient_like_the_reference(name):
    g, task = fixture(name)[0], task_of(name)
    for tag, clamp in (("", False), ("_c", True)):
        set_clamp(task, clamp)
        try:
            for suf in ("", "_edge"):
                q = dev(g[f"q{suf}"]).requires_grad_(True)
                cost = task.compute_collision_cost(q)
                got, ref = cost.detach().cpu().numpy(), g[f"cost{tag}{suf}"]
                assert got.size == ref.size and rel_err(got.reshape(ref.shape), ref) < TOL_C, (tag, suf)
                cost.sum().backward()
                gq = q.grad.cpu().numpy()
                assert grad_close(gq, g[f"gq{tag}{suf}"]), (tag, suf)
                if name == "ties" and suf == "_edge":                  # exact ties: exact gradients, the hinge at exactly 0 included
                    rows = slice(TIE_ROWS.start, HINGE_ROWS.stop) if clamp else TIE_ROWS
                    np.testing.assert_array_equal(gq.reshape(-1, 2)[rows], g[f"gq{tag}{suf}"].reshape(-1, 2)[rows])
                    if clamp:
                        assert (got.reshape(-1)[HINGE_ROWS] == 0).all() and (gq.reshape(-1, 2)[HINGE_ROWS] == 0).all()
                with torch.no_grad():
                    np.testing.assert_array_equal(task.compute_collision_cost(q).cpu().numpy(), got)
        finally:
            set_clamp(task, False)


@pytest.mark.parametrize("name", NAMES)
def test_booleans_at_both_margins(name):
    g, task = fixture(name)[0], task_of(name)
    for suf in ("", "_edge"):
        q = dev(g[f"q{suf}"])
        np.testing.assert_array_equal(task.compute_collision(q).cpu().numpy().reshape(g[f"coll{suf}"].shape), g[f"coll{suf}"])
        np.testing.assert_array_equal(task.compute_collision(q, margin=0.0).cpu().numpy().reshape(g[f"coll0{suf}"].shape), g[f"coll0{suf}"])


@pytest.mark.parametrize("name", NAMES)
def test_compute_sdf_and_every_object(name):
    g, env = fixture(name)[0], env_of(name)
    objs = list(env.obj_fixed_list or []) + list(env.obj_extra_list or [])
    for suf in ("", "_edge"):
        x = dev(g[f"q{suf}"]).requires_grad_(True)
        sdf = env.compute_sdf(x)
        assert sdf.shape == g[f"sdf{suf}"].shape and rel_err(sdf.detach().cpu().numpy(), g[f"sdf{suf}"]) < TOL_C
        sdf.sum().backward()
        assert grad_close(x.grad.cpu().numpy(), g[f"gsdf{suf}"])
        if name == "ties" and suf == "_edge":
            np.testing.assert_array_equal(x.grad.cpu().numpy()[TIE_ROWS], g[f"gsdf{suf}"][TIE_ROWS])
        for k, o in enumerate(objs):                                    # ObjectField.compute_signed_distance, object by object
            p = dev(g[f"q{suf}"]).reshape(-1, 2).requires_grad_(True)
            d = o.compute_signed_distance(p)
            assert rel_err(d.detach().cpu().numpy(), g[f"obj_sdf{suf}"][:, k]) < TOL_C, (suf, k)
            d.sum().backward()
            assert grad_close(p.grad.cpu().numpy(), g[f"obj_gsdf{suf}"][:, k]), (suf, k)


@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_at_sampled_cells_and_tie_nodes(name):
    g, env = fixture(name)[0], env_of(name)
    gm = env.grid_map_sdf_obj_fixed
    assert tuple(gm.sdf_tensor.shape) == tuple(g["grid_dims"]) and tuple(gm.grad_sdf_tensor.shape) == tuple(g["grid_dims"]) + (2,)
    assert gm.sdf_tensor.shape[0] != gm.sdf_tensor.shape[1]
    for cells, sdf_ref, grad_ref in ((g["grid_cells"], g["grid_sdf"], g["grid_grad"]), (g["grid_tie_cells"], g["grid_tie_sdf"], g["grid_tie_grad"])):
        if len(cells) == 0:
            continue
        sdf = gm.sdf_tensor[cells[:, 0], cells[:, 1]].cpu().numpy()
        grad = gm.grad_sdf_tensor[cells[:, 0], cells[:, 1]].cpu().numpy()
        assert rel_err(sdf, sdf_ref) < TOL_C
        assert grad_close(grad, grad_ref)
    if name == "gridtie":
        cells = g["grid_tie_cells"]
        assert len(cells) >= 40                                              # the nodes x == 0, equidistant from the two spheres
        grad = gm.grad_sdf_tensor[cells[:, 0], cells[:, 1]].cpu().numpy()
        np.testing.assert_array_equal(grad[:, 0], np.zeros(len(cells), np.float32))       # the mirrored x components average to exactly 0
        assert (g["grid_tie_grad"][:, 0] == 0).all()                       # "first wins" would leave gx = -dx / |d| != 0 there


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_validation(name):
    g, task = fixture(name)[0], task_of(name)
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


@pytest.mark.parametrize("name,moved", [("posed", 1), ("gridposed", 2)])
def test_moved_object_equals_a_fresh_task(name, moved):
    """set_position_orientation on an object of a live task (an analytic object: a grid keeps its recorded cells, as the reference's does):
    the next evaluations equal those of a task built fresh with that pose -- the 2-D handles are rebuilt, not reused."""
    g, scene = fixture(name)
    pos, ori = np.array([0.15, -0.35, 0.2], np.float32), np.array([0.8, 0.1, -0.2, 1.3], np.float32)
    live_env = hp.planar_build_env(tra, scene, TA)
    live = tra.PlanningTask(env=live_env, robot=tra.RobotPointMass(tensor_args=TA), tensor_args=TA)
    q, trajs = dev(g["q"]), dev(g["trajs"])
    before = live.compute_collision_cost(q).clone()                      # builds the handles for the old pose
    live.compute_collision(q), live_env.compute_sdf(q), live.get_trajs_collision_and_free(trajs, return_indices=True)
    objs = list(live_env.obj_fixed_list or []) + list(live_env.obj_extra_list or [])
    assert not scene["grid_on"] or scene["objects"][moved]["extra"]
    objs[moved].set_position_orientation(pos=pos, ori=ori)
    fresh_objects = [dict(o, pos=pos, ori=ori) if k == moved else o for k, o in enumerate(scene["objects"])]
    fresh_env = hp.planar_build_env(tra, scene, TA, objects=fresh_objects)
    fresh = tra.PlanningTask(env=fresh_env, robot=tra.RobotPointMass(tensor_args=TA), tensor_args=TA)
    after = live.compute_collision_cost(q)
    assert not torch.equal(before, after)
    np.testing.assert_array_equal(after.cpu().numpy(), fresh.compute_collision_cost(q).cpu().numpy())
    np.testing.assert_array_equal(live.compute_collision(q).cpu().numpy(), fresh.compute_collision(q).cpu().numpy())
    np.testing.assert_array_equal(live_env.compute_sdf(q).cpu().numpy(), fresh_env.compute_sdf(q).cpu().numpy())
    a, b = live.get_trajs_collision_and_free(trajs, return_indices=True), fresh.get_trajs_collision_and_free(trajs, return_indices=True)
    for u, v in zip(a[1:], b[1:]):
        if u is None or v is None:
            assert u is None and v is None
        else:
            np.testing.assert_array_equal(u.cpu().numpy(), v.cpu().numpy())
    # and both agree with fp64 at the new pose
    m = margin_of(g)
    grid = grid64_of(live_env)
    ana = [o for o in fresh_objects if o["extra"] or grid is None]
    c64 = hp.planar64(ana, g["q"], m, ws=tuple(scene["limits"]), grid=grid)[0]
    assert rel_err(after.cpu().numpy().reshape(-1), c64) < TOL_C


# ---------------------------------------------------------------------------------------------------------------------------
# seeded batches of every compiled variant against fp64, through ops
# ---------------------------------------------------------------------------------------------------------------------------
def grid64_of(env):
    gm = env.grid_map_sdf_obj_fixed
    if gm is None:
        return None
    return dict(sdf=gm.sdf_tensor.cpu().numpy(), grad=gm.grad_sdf_tensor.cpu().numpy(), lo=gm.limits[0].numpy(), md=gm.map_dim.numpy())


def variant(name, use_grid, use_ana, use_ws):
    """(Scene2DHandle, fp64 arguments) of one compiled variant (grid, analytic, workspace) on a synthetic scene"""
    g, scene = fixture(name)
    env = env_of(name)
    m = margin_of(g)
    gm = env.grid_map_sdf_obj_fixed
    assert not use_grid or gm is not None
    if use_ana:      # the analytic objects: after a grid only the extra ones (EnvBase.get_df_obj_list), without a grid all of them
        pick = [k for k, o in enumerate(scene["objects"]) if (o["extra"] if use_grid else True)]
    else:
        pick = []
    all_objs = list(env.obj_fixed_list or []) + list(env.obj_extra_list or [])
    objects, prims = planar_tables([all_objs[k] for k in pick])
    ws = (scene["limits"][0], scene["limits"][1]) if use_ws else None
    h = ops.Scene2DHandle(objects, prims, DEV, grid=gm.planar_grid(DEV) if use_grid else None, ws=ws, margin=float(m))
    return h, dict(objects=[scene["objects"][k] for k in pick], margin=m, ws=ws, grid=grid64_of(env) if use_grid else None)


def batch_of(name):
    if ("batch", name) not in _cache:
        g, scene = fixture(name)
        ladder = [o for o in scene["objects"] if o["extra"] or not scene["grid_on"]]
        _cache[("batch", name)] = hp.planar_batch(ladder, scene["limits"], hp.planar_margins(margin_of(g)), hp.PLANAR_BATCH_N, int(g["batch_seed"]))
    return _cache[("batch", name)]


VARIANTS = [("ties", False, True, True), ("ties", False, True, False), ("posed", False, True, True), ("posed", False, True, False),
            ("sharp", False, True, True), ("sharp", False, True, False),
            ("gridtie", True, False, True), ("gridtie", True, False, False), ("gridthin", True, False, True), ("gridthin", True, False, False),
            ("gridposed", True, True, True), ("gridposed", True, True, False), ("gridposed", True, False, True),
            ("gridposed", False, True, True),                                       # every object analytic, the tilted ones included
            ("posed", False, False, True)]                                          # workspace only


@pytest.mark.parametrize("name,use_grid,use_ana,use_ws", VARIANTS)
@pytest.mark.parametrize("clamp", [False, True])
def test_variant_cost_and_gradient_against_fp64(name, use_grid, use_ana, use_ws, clamp):
    h, a = variant(name, use_grid, use_ana, use_ws)
    g = fixture(name)[0]
    band = 2.0 * float(g["band_measured"])
    qb = batch_of(name)
    c64, g64, s64, _ = hp.planar64(a["objects"], qb, a["margin"], ws=a["ws"], grid=a["grid"], clamp=clamp)
    # under clamp_sdf the ladder sits on relu's kink by construction: a row within the band of a hinge is not exempt, it must carry one
    # of the one-sided fp64 gradients at its own q (each field's hinge clamped or not); every other row meets the usual bound
    decided = hp.planar_hinge_decided(s64, qb, a["ws"], float(a["margin"]), band) if clamp else np.ones(len(qb), bool)
    sides = hp.planar_hinge_sides64(a["objects"], qb[~decided], float(a["margin"]), band, ws=a["ws"], grid=a["grid"]) if clamp else None

    def oracle(qp):          # fp64 gradient at the fp64 probe points (a grid's cell is taken at the fp32-rounded probe)
        return hp.planar64(a["objects"], qp, a["margin"], ws=a["ws"], grid=a["grid"], clamp=clamp)[1]

    for n in SIZES:
        q = dev(qb[:n])
        cost, grad = ops.planar_cost_grad(h, q, clamp=clamp, want_grad=True)
        cost_only, none = ops.planar_cost_grad(h, q, clamp=clamp, want_grad=False)
        assert none is None and cost.shape == (n,) and grad.shape == (n, 2)
        np.testing.assert_array_equal(cost_only.cpu().numpy(), cost.cpu().numpy())            # the variant without the gradient output
        assert np.abs(cost.cpu().numpy() - c64[:n]).max() <= TOL_C * np.abs(c64).max(), n         # on the whole batch's scale at every prefix size (rel_err's measure at the full size)
        dn = decided[:n]
        if (~dn).any():
            k = int((~dn).sum())                                          # the undecided rows of the prefix are the first k of all
            ok = hp.planar_rows_match_any(grad.cpu().numpy()[~dn], sides[:, :k])
            assert ok.all(), (n, qb[:n][~dn][~ok][:4], grad.cpu().numpy()[~dn][~ok][:4])
        got, ref = grad.cpu().numpy()[dn], g64[:n][dn]
        if len(ref) == 0:
            continue
        bad = hp.planar_bad_rows(got, ref) if np.abs(ref).max() > 0 else np.abs(got).max(-1) > 0
        assert bad.sum() <= n // 10000, (n, int(bad.sum()), np.flatnonzero(bad)[:8])
        if bad.any():
            assert hp.kink_rows_ok(got, ref, qb[:n][dn], oracle, bad, max_rows=n // 10000, radius=1e-7)
        if (~bad).any() and np.abs(ref[~bad]).max() > 0:
            assert grad_close(got[~bad], ref[~bad], scale=np.abs(ref).max() / np.abs(ref[~bad]).max()), n
    cost, grad = ops.planar_cost_grad(h, torch.empty(0, 2, device=DEV), clamp=clamp)
    assert cost.shape == (0,) and grad.shape == (0, 2)


@pytest.mark.parametrize("name,use_grid,use_ana,use_ws", VARIANTS)
def test_variant_booleans_and_distances_against_fp64(name, use_grid, use_ana, use_ws):
    h, a = variant(name, use_grid, use_ana, use_ws)
    g = fixture(name)[0]
    band = 2.0 * float(g["band_measured"])
    qb = batch_of(name)
    _, _, s64, _ = hp.planar64(a["objects"], qb, a["margin"], ws=None, grid=a["grid"], want_grad=False)
    d64 = hp.planar_nearest64(a["objects"], qb, a["ws"], a["grid"])
    m_scene, m_over, m_zero = hp.planar_margins(a["margin"])
    for n in SIZES:
        q = dev(qb[:n])
        if s64.shape[1]:
            sdf, gs = ops.planar_sdf_points(h, q, want_grad=True)
            assert sdf.shape == (n, s64.shape[1]) and gs.shape == (n, s64.shape[1], 2)
            assert np.abs(sdf.cpu().numpy() - s64[:n]).max() <= TOL_C * np.abs(s64).max(), n
            np.testing.assert_array_equal(ops.planar_sdf_points(h, q).cpu().numpy(), sdf.cpu().numpy())
        for margin, mm in ((None, m_scene), (m_scene, m_scene), (m_over, m_over), (0.0, m_zero)):      # NaN default, then explicit overrides
            coll = ops.planar_collision(h, q, margin=margin).cpu().numpy()
            assert coll.shape == (n,) and coll.dtype == np.bool_
            far = np.abs(d64[:n] - mm) > band
            np.testing.assert_array_equal(coll[far], (d64[:n] < mm)[far], err_msg=f"n {n} margin {margin}")
    if use_ana or use_ws:          # the ladder left decided samples close to each threshold, on both sides (a grid alone has no ladder)
        for mm in (m_scene, m_over, m_zero):
            above = ((d64 - mm > band) & (d64 - mm <= 10 * band)).sum()
            below = ((mm - d64 > band) & (mm - d64 <= 10 * band)).sum()
            assert above >= MIN_DECIDED and below >= MIN_DECIDED, (mm, int(above), int(below))
    assert ops.planar_collision(h, torch.empty(0, 2, device=DEV)).shape == (0,)
    if s64.shape[1]:
        assert ops.planar_sdf_points(h, torch.empty(0, 2, device=DEV)).shape == (0, s64.shape[1])


@pytest.mark.parametrize("name,use_grid", [("gridposed", True), ("posed", False)])
def test_via_points_bit_equal_to_interpolate_then_test(name, use_grid):
    h, a = variant(name, use_grid, True, True)
    g, scene = fixture(name)
    lo, hi = scene["limits"].astype(np.float64)
    rng = np.random.default_rng(int(g["batch_seed"]) + 7)
    hits = total = 0
    for T in (1, 3, 47):
        for H in (2, 3, 64):
            for S in (2, 3, 4, 5):
                x = rng.uniform(lo - 0.1, hi + 0.1, (T, H, 2))
                trajs = dev(np.concatenate([x, rng.normal(0, 1, (T, H, S - 2))], -1).astype(np.float32))
                for n_interp in (1, 5, 7):
                    for margin in (None, 0.0):
                        fused = ops.planar_collision_via(h, trajs, n_interp, margin=margin)
                        pts = ops.interpolate_traj_via_points(trajs, n_interp)
                        assert fused.shape == (T, (H - 1) * n_interp) == tuple(pts.shape[:2])
                        two = ops.planar_collision(h, pts[..., :2].contiguous(), margin=margin)
                        np.testing.assert_array_equal(fused.cpu().numpy(), two.cpu().numpy(), err_msg=f"{T} {H} {S} {n_interp} {margin}")
                        hits, total = hits + int(fused.sum()), total + fused.numel()
    assert 0 < hits < total                                             # both outcomes occur over the whole sweep


# ---------------------------------------------------------------------------------------------------------------------------
# the whole grid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_NAMES)
def test_every_grid_cell_against_fp64(name):
    g, scene = fixture(name)
    env = env_of(name)
    gm = env.grid_map_sdf_obj_fixed
    nx, ny = gm.sdf_tensor.shape
    lim = scene["limits"]
    xs = torch.linspace(float(lim[0][0]), float(lim[1][0]), nx, dtype=torch.float32).numpy()          # the reference's nodes
    ys = torch.linspace(float(lim[0][1]), float(lim[1][1]), ny, dtype=torch.float32).numpy()
    nodes = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    fixed = [o for o in scene["objects"] if not o["extra"]]
    s64, g64 = hp.planar_grid64(fixed, nodes)
    sdf, grad = gm.sdf_tensor.cpu().numpy().reshape(-1), gm.grad_sdf_tensor.cpu().numpy().reshape(-1, 2)
    assert np.abs(sdf - s64).max() <= TOL_C * np.abs(s64).max()
    bad = hp.planar_bad_rows(grad, g64)
    assert bad.sum() <= len(nodes) // 10000, (int(bad.sum()), nodes[bad][:5])
    if bad.any():
        assert hp.kink_rows_ok(grad, g64, nodes, lambda p: hp.planar_grid64(fixed, p)[1], bad, max_rows=len(nodes) // 10000, radius=1e-7)
    assert grad_close(grad[~bad], g64[~bad])
    # the reference-shaped tensors are views of the packed cells
    assert gm.cells.shape == (nx, ny, 4) and gm.sdf_tensor.data_ptr() == gm.cells.data_ptr()
    assert gm.grad_sdf_tensor.data_ptr() == gm.cells.data_ptr() + 4 and gm.sdf_tensor._base is gm.cells and gm.grad_sdf_tensor._base is gm.cells
    assert (gm.cells[..., 3] == 0).all()
    if name == "gridtie":
        tie = g["grid_tie_cells"]
        flat = tie[:, 0] * ny + tie[:, 1]
        assert len(tie) > 0 and (nodes[flat, 0] == 0).all()
        np.testing.assert_array_equal(grad[flat, 0], 0.0)
        assert np.abs(grad[flat] - g64[flat]).max() < 1e-6


@pytest.mark.parametrize("dims", [(1, 7), (5, 1), (1, 1)])
def test_precompute_with_an_axis_of_one(dims):
    g, scene = fixture("gridposed")
    env = env_of("gridposed")
    fixed = [o for o in scene["objects"] if not o["extra"]]
    objects, prims = planar_tables(env.obj_fixed_list)
    h = ops.Scene2DHandle(objects, prims, DEV)
    lim = scene["limits"]
    cells = ops.grid2d_precompute(h, dims, lim[0], lim[1]).cpu().numpy()
    assert cells.shape == dims + (4,)
    xs = torch.linspace(float(lim[0][0]), float(lim[1][0]), dims[0], dtype=torch.float32).numpy()      # one node: the lower limit
    ys = torch.linspace(float(lim[0][1]), float(lim[1][1]), dims[1], dtype=torch.float32).numpy()
    nodes = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    s64, g64 = hp.planar_grid64(fixed, nodes)
    assert np.abs(cells[..., 0].reshape(-1) - s64).max() <= TOL_C * np.abs(s64).max()
    assert grad_close(cells[..., 1:3].reshape(-1, 2), g64)
    # a lookup in such a grid clamps every point to the single row / column
    hg = ops.Scene2DHandle([], np.zeros((0, 6), np.float32), DEV,
                           grid=dict(cells=torch.as_tensor(cells, device=DEV).contiguous(), lim_min=lim[0], map_dim=np.abs(lim[1] - lim[0])))
    q = batch_of("gridposed")[:257]
    idx = hp.planar_grid_index(q, lim[0], np.abs(lim[1] - lim[0]), dims)
    np.testing.assert_array_equal(ops.planar_sdf_points(hg, dev(q)).cpu().numpy()[:, 0], cells[idx[:, 0], idx[:, 1], 0])


# ---------------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------------
def capacity_scene(n_obj, per_obj, seed=5):
    rng = np.random.default_rng(seed)
    objs = []
    for k in range(n_obj):
        kind = k % 3
        c = rng.uniform(-0.3, 0.3, (per_obj, 2)).astype(np.float32)
        ab = np.stack([rng.uniform(0.03, 0.08, per_obj), rng.uniform(0.03, 0.08, per_obj) * (kind != 0)], 1).astype(np.float32)
        ang = rng.uniform(-np.pi, np.pi)
        objs.append(dict(pos=np.array([*rng.uniform(-0.7, 0.7, 2), 0.0], np.float32), extra=False, name=f"o{k}",
                         ori=np.array([np.cos(ang / 2), 0, 0, np.sin(ang / 2)], np.float32) * np.float32(1 + k % 2),
                         fields=[(kind, c, ab)]))
    return dict(limits=np.array([[-1, -1], [1, 1]], np.float32), cell=0.01, grid_on=False, objects=objs)


def test_capacity_64_objects_256_primitives():
    scene = capacity_scene(64, 4)
    env = hp.planar_build_env(tra, scene, TA)
    objects, prims = planar_tables(env.obj_fixed_list)
    assert len(objects) == 64 and len(prims) == 256
    m = np.float32(0.02)
    ws = (scene["limits"][0], scene["limits"][1])
    h = ops.Scene2DHandle(objects, prims, DEV, ws=ws, margin=float(m))
    q = np.random.default_rng(11).uniform(-1.1, 1.1, (4099, 2)).astype(np.float32)
    c64, g64, s64, _ = hp.planar64(scene["objects"], q, m, ws=ws)
    cost, grad = ops.planar_cost_grad(h, dev(q))
    assert np.abs(cost.cpu().numpy() - c64).max() <= TOL_C * np.abs(c64).max()
    sdf = ops.planar_sdf_points(h, dev(q)).cpu().numpy()
    assert sdf.shape == (4099, 64) and np.abs(sdf - s64).max() <= TOL_C * np.abs(s64).max()
    bad = hp.planar_bad_rows(grad.cpu().numpy(), g64)
    assert hp.kink_rows_ok(grad.cpu().numpy(), g64, q, lambda p: hp.planar64(scene["objects"], p, m, ws=ws)[1], bad,
                           max_rows=0, radius=1e-7)


def test_past_the_capacity_raises():
    for n_obj, per in ((65, 1), (1, 257)):
        scene = capacity_scene(n_obj, per)
        env = hp.planar_build_env(tra, scene, TA)
        objects, prims = planar_tables(env.obj_fixed_list)
        with pytest.raises(NotImplementedError, match="at most 64 / 256"):
            ops.Scene2DHandle(objects, prims, DEV)
        with pytest.raises(NotImplementedError, match="at most 64 / 256"):
            env.compute_sdf(torch.zeros(3, 2, device=DEV))

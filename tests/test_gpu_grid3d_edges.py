"""The 3-D voxel-grid scene path (k_grid_precompute, k_grid_pack, grid_cell / grid_record / grid_sdf and every kernel that reads a
scene through them) off the two cubic, origin-centred grids the rest of the suite uses.

On a cubic grid that is symmetric about the origin, whose dimensions are multiples of four and whose objects sit unrotated at the
origin, a swapped brick count, a dimension or a limit of the wrong axis, x-major against z-major packing, addressed brick padding
or an ignored object pose all compute the right numbers.  Here

  1. "address" grids -- every cell stores a distance and a gradient of its own, the dimensions are (5, 6, 7), (4, 8, 12), (7, 4, 9),
     (2, 3, 130), three with an axis of one cell, (1, 1, 1) and the cubic control, the limits differ on every axis -- are read at every
     cell's centre, on and one ulp either side of every face, at signed zeros and from one ulp to 1000 m outside, through
     sdf_points, cost_fields and collision_fields (generated and table-driven), alone and next to an analytic sphere object; the
     expected cell is GridMapSDF.get_sdf's own fp32 arithmetic in numpy, and the values read must be that cell's;
  2. the fused rollouts run on two such grids that part of the arm leaves: two-step rule on the returned positions, gradients against
     the fp64 oracle where fp32 and fp64 agree on the cell;
  3. the precompute is held to the reference's own nodes, torch.linspace per axis (an axis of one node is [lo]), on posed objects,
     independently of the oracle's precompute, and its output is read back;
  4. one non-cubic grid recorded from the reference's GridMapSDF (tests/golden/cost_grid3d_aniso.npz) pins all of it.

Tolerances: a distance recovered from a cost, (K margin - cost) / K, to TOL_C of the largest stored distance; stored gradients and
q-gradients to helpers.grad_close; everything read without arithmetic, array_equal.  Two cells of an address grid differ by
(vhi - vlo) / n_cells: at least 250 x that cost tolerance on the grids of up to 780 cells, 25 x on the 8000-cell control (8000 distinct
values cannot be 100 tolerances apart inside +-1; there the gradients, which differ by 1e-3 and more between any two cells, and the
exact sdf_points comparison carry the address).

What these tests found besides the one-node axis: the generated units grant the compiler reassociation (`#pragma clang fp`), and it
turned the index expression into ((p - lim_min) * cmap_dim) / map_dim, which rounds up to the next integer at points within an ulp of
a cell face -- k_fields / k_collf and the generated rollouts then read the neighbouring cell (24 of 646 points on (5, 6, 7), 152 of
2620 on (2, 3, 130), 16 of 8940 on the cubic control) where k_sdf_points and the table-driven kernels read the reference's.
grid_axis_cell now pins the reference's operation order.
"""
import numpy as np
import pytest
import torch

import helpers as H
from helpers import (ADDRESS_DIMS, ADDRESS_HI, ADDRESS_LO, ADDRESS_MARGIN, ROLLOUT_GRID_DIMS, ROLLOUT_HI, ROLLOUT_LO,
                     address_coverage, address_grid, address_points, address_spec, gold, grad_close, grid_index,
                     grid_precompute_check, linspace_nodes, model, rel_err, scene_min64, scene_only_spec)
from oracle.oracle import Oracle
from torch_robotics_amd import ops
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS
from torch_robotics_amd.costmodel import CostModelSpec, grid_object, make_object, sphere_prims

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL_C = 1e-5
MG = float(ADDRESS_MARGIN)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _grid_only_cm(grid):
    spec = CostModelSpec(n_links_in=11, objects=[grid_object()])
    spec.grid = dict(grid)
    spec.validate()
    return ops.CostHandle(spec, DEV)


def _check_fields(cm, spec, pts, s_ref, g_ref, tol_s, what, grad_rows=None):
    """cost_fields / collision_fields with all 11 link columns at the query point, generated and table-driven: the distance recovered
    from the cost, the gradient of every collision-link column (minus the distance's gradient: the cost is margin - distance) and of
    every other column (zero), the boolean.  Returns the worst distance error."""
    K = len(spec.obj_link_idx)
    pos = _dev(np.repeat(pts[:, None, :], 11, axis=1))
    rows = np.ones(len(pts), bool) if grad_rows is None else grad_rows
    other = np.setdiff1d(np.arange(11), np.asarray(spec.obj_link_idx))
    worst = 0.0
    for generated in (True, False):
        cm.enable_specialized(generated)
        hit = ops.collision_fields(cm, FIELD_OBJECTS, pos).cpu().numpy().astype(bool)
        cost, g = ops.cost_fields(cm, FIELD_OBJECTS, pos, want_grad=True)
        torch.cuda.synchronize()
        s = (K * MG - cost.cpu().numpy().astype(np.float64)) / K
        err = np.abs(s - s_ref)
        worst = max(worst, float(err.max()))
        assert err.max() <= tol_s, f"{what} generated={generated}: distance off by {err.max():.3g} at point {pts[np.argmax(err)]}"
        g = g.cpu().numpy()
        gl = g[:, np.asarray(spec.obj_link_idx), :]
        assert grad_close(gl[rows], np.repeat(-g_ref[rows, None, :], K, axis=1)), f"{what} generated={generated}: gradient"
        assert (g[:, other, :] == 0).all(), f"{what} generated={generated}: a column outside the collision links has a gradient"
        np.testing.assert_array_equal(hit, s_ref < MG, err_msg=f"{what} generated={generated}: booleans")
    cm.enable_specialized(True)
    return worst


@pytest.mark.parametrize("dims", ADDRESS_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_address_grid_lookup(dims):
    """part 1, the grid alone: the cell read is the cell of the reference's fp32 index arithmetic, for every cell, face and clamp"""
    grid = address_grid(dims, ADDRESS_LO, ADDRESS_HI)
    pts = address_points(dims, ADDRESS_LO, ADDRESS_HI)
    assert len(pts) <= 4133 or tuple(dims) == (20, 20, 20)
    c = address_coverage(pts, grid)
    s_ref, g_ref = grid["sdf"][c[:, 0], c[:, 1], c[:, 2]], grid["grad"][c[:, 0], c[:, 1], c[:, 2]]
    # two cells differ by at least 100 cost tolerances (25 on the control, see the module docstring), none is near the margin
    tol_s = TOL_C * float(np.abs(grid["sdf"]).max())
    if int(np.prod(dims)) > 1:
        assert np.diff(np.sort(grid["sdf"].ravel())).min() >= (25 if tuple(dims) == (20, 20, 20) else 100) * tol_s
    assert np.abs(grid["sdf"] - MG).min() > 1e-4
    s, g = ops.sdf_points(_grid_only_cm(grid), _dev(pts), want_grad=True)
    s, g = s.cpu().numpy(), g.cpu().numpy()
    bad = np.flatnonzero(s[:, 0] != s_ref)
    assert len(bad) == 0, (f"{dims}: {len(bad)} points read another cell; first {pts[bad[0]]!r}: expected cell {c[bad[0]]}, got the value of "
                           f"cell {np.argwhere(grid['sdf'] == s[bad[0], 0])}")
    np.testing.assert_array_equal(g[:, 0, :], g_ref)
    spec = address_spec(grid)
    worst = _check_fields(ops.CostHandle(spec, DEV), spec, pts, s_ref.astype(np.float64), g_ref.astype(np.float64), tol_s, f"grid {dims}")
    print(f"address grid {dims}: {len(pts)} points, sdf_points exact, worst distance recovered from the cost off by {worst:.3g} (allowed {tol_s:.3g})")


@pytest.mark.parametrize("dims", ADDRESS_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_address_grid_next_to_spheres(dims):
    """part 1, the minimum over the grid and an analytic sphere object: each of the two spheres and the grid win at least a tenth of
    the points.  helpers.address_sphere_case leaves out points within 1e-4 of a tie between grid and spheres or of the margin (the sphere
    distances are continuous, the test cannot choose them) before the coverage is asserted."""
    grid, cw, r, pts, sg, ds, us = H.address_sphere_case(dims)
    c = address_coverage(pts, grid)
    win = np.where(sg < ds.min(1), 2, np.argmin(ds, 1))
    assert min((win == k).mean() for k in range(3)) >= 0.1, [(win == k).mean() for k in range(3)]
    assert np.abs(grid["sdf"] - MG).min() > 1e-4
    g_grid = grid["grad"][c[:, 0], c[:, 1], c[:, 2]].astype(np.float64)
    rows = np.arange(len(pts))
    s_ref = np.minimum(sg, ds.min(1))
    g_ref = np.where((win == 2)[:, None], g_grid, us[rows, np.argmin(ds, 1)])
    spec = address_spec(grid, [make_object(sphere_prims(cw, r))])
    cm = ops.CostHandle(spec, DEV)
    s, g = ops.sdf_points(cm, _dev(pts), want_grad=True)
    s, g = s.cpu().numpy(), g.cpu().numpy()
    np.testing.assert_array_equal(s[:, 0], sg.astype(np.float32))                    # the grid's column: the cell as stored
    np.testing.assert_array_equal(g[:, 0, :], g_grid.astype(np.float32))
    # the sphere object's column: fp32 rounding of a distance of up to 1000 m
    assert (np.abs(s[:, 1] - ds.min(1)) <= 2e-6 * np.maximum(1.0, np.abs(ds.min(1)))).all()
    tol_s = TOL_C * float(max(np.abs(grid["sdf"]).max(), np.abs(s_ref).max()))
    worst = _check_fields(cm, spec, pts, s_ref, g_ref, tol_s, f"grid {dims} + spheres")
    print(f"address grid {dims} + spheres: {len(pts)} points, winners (sphere 0, sphere 1, grid) "
          f"{[round(float((win == k).mean()), 2) for k in range(3)]}, worst distance off by {worst:.3g} (allowed {tol_s:.3g})")


# ---------------------------------------------------------------------------------------------------------------------------
# part 2: fused rollouts
# ---------------------------------------------------------------------------------------------------------------------------
def _near_face_or_margin(pos, grid, s_links):
    """a boolean may differ between two launches where a distance lies within 1e-6 of its margin or -- the positions of two kernels
    differing in their last ulp -- where a link coordinate lies within 1e-6 of a cell face"""
    return (np.abs(s_links - MG) < 1e-6).any() or not H.off_face_rows(pos[None].astype(np.float64), grid, band=1e-6)[0]


@pytest.mark.parametrize("base", list(H.ROLLOUT_BASES))
@pytest.mark.parametrize("dims", ROLLOUT_GRID_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_rollouts_on_a_non_cubic_grid(dims, base):
    """rollout_cost_grad and rollout_collision, generated unit and table-driven, on an address grid that part of the arm leaves"""
    grid = address_grid(dims, ROLLOUT_LO, ROLLOUT_HI, seed=5)
    spec = address_spec(grid, full=True)
    m = model("panda_arm_no_gripper")
    if H.ROLLOUT_BASES[base] is not None:
        m.set_base_pose(H.ROLLOUT_BASES[base])
    h, cm = ops.ModelHandle(m), ops.CostHandle(spec, DEV)
    h.set_base_pose(m.base_R, m.base_t)
    orc = Oracle(m, spec)
    allf = FIELD_SELF | FIELD_OBJECTS | FIELD_WS
    oli = np.asarray(spec.obj_link_idx)
    K = len(oli)
    worst = dict(cost=0.0, two_step=0.0, judged=1.0)
    for n in H.ROLLOUT_NS:
        q = H.panda_q(n, 100 + n)
        qd = _dev(q)
        for w in ((0, 1, 0, 0), (1, 1, 1, 1)):
            p64, c64, g64 = orc.rollout(q.astype(np.float64), w, "f64")
            judged = H.off_face_rows(p64, grid)
            worst["judged"] = min(worst["judged"], float(judged.mean()))
            assert judged.mean() >= 0.95, (dims, base, n, judged.mean())
            lo, hi = grid["lim_min"].astype(np.float64), (grid["lim_min"] + grid["map_dim"]).astype(np.float64)
            if n >= 63:
                outside = ((p64[:, oli] < lo) | (p64[:, oli] > hi)).any(-1)
                assert outside.any(1).mean() > 0.3 and (~outside).any(1).mean() > 0.3          # part of the arm outside the limits, part inside
            for generated in (True, False):
                h.enable_specialized(generated)
                pos, cost, gq = ops.rollout_cost_grad(h, cm, w, qd)
                assert ops.last_dispatch() == ("generated" if generated else "table-driven")
                assert not ops.last_plan_specialized()                                         # a grid scene is not scene_is_fast
                pos_np, cost_np, gq_np = pos.cpu().numpy(), cost.cpu().numpy().astype(np.float64), gq.cpu().numpy()
                what = f"grid {dims} base {base} n {n} weights {w} generated {generated}"
                assert np.abs(pos_np - p64).max() < 2e-6, what
                # the two-step rule: the fields on the positions the rollout itself returned
                if w == (0, 1, 0, 0):
                    two = ops.cost_fields(cm, FIELD_OBJECTS, pos).cpu().numpy().astype(np.float64)
                else:
                    two = (ops.cost_fields(cm, allf, pos) + ops.ee_cost(cm, ops.fk_forward(h, qd)[:, spec.ee_link])).cpu().numpy().astype(np.float64)
                e2 = rel_err(cost_np, two)
                worst["two_step"] = max(worst["two_step"], e2)
                assert e2 < TOL_C, f"{what}: cost against cost_fields on the returned positions {e2:.3g}"
                ec = rel_err(cost_np[judged], c64[judged])
                worst["cost"] = max(worst["cost"], ec)
                assert ec < TOL_C, f"{what}: cost against the fp64 oracle {ec:.3g}"
                assert grad_close(gq_np[judged], g64[judged]), what
                for fl in (FIELD_OBJECTS, allf):
                    want = ops.collision_fields(cm, fl, pos).cpu().numpy().astype(bool)
                    got = ops.rollout_collision(h, cm, fl, qd).cpu().numpy().astype(bool)
                    bad = np.flatnonzero(got != want)
                    assert len(bad) <= max(1, n // 2000), (what, fl, len(bad))
                    for b in bad:
                        c = grid_index(pos_np[b, oli], grid["lim_min"], grid["map_dim"], dims)
                        assert _near_face_or_margin(pos_np[b, oli], grid, grid["sdf"][c[:, 0], c[:, 1], c[:, 2]]), (what, fl, int(b))
            h.enable_specialized(True)
    print(f"rollouts on grid {dims}, base {base}: worst rel. cost error against fp64 {worst['cost']:.3g}, against the two-step path "
          f"{worst['two_step']:.3g}, smallest judged share {worst['judged']:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# part 3: the precompute at torch.linspace's nodes, and its output read back
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ADDRESS_DIMS[:-1], ids=lambda d: "x".join(map(str, d)))
def test_grid_precompute_at_linspace_nodes(dims):
    """k_grid_precompute on posed objects (a translated sphere object, a translated rounded-box object rotated about a tilted axis)
    against fp64 distances at the reference's nodes -- an axis of one node sits at the LOWER limit --, then a round trip: the
    kernel's own output as the cost model's grid, read at 4133 points of which a quarter lie outside the limits."""
    spec = scene_only_spec(H.posed_scene_objects())
    cm, orc = ops.CostHandle(spec, DEV), Oracle(model("panda_arm_no_gripper"), spec)
    nodes = linspace_nodes(dims, ADDRESS_LO, ADDRESS_HI)
    ref_s, ref_g = scene_min64(orc, nodes)
    sdf, grad = ops.grid_precompute(cm, dims, ADDRESS_LO, ADDRESS_HI)
    assert tuple(sdf.shape) == tuple(dims) and tuple(grad.shape) == tuple(dims) + (3,)
    grid_precompute_check(sdf.cpu().numpy(), grad.cpu().numpy(), ref_s, ref_g, nodes, orc, f"kernel {dims}")
    assert np.ptp(ref_s) > 0.05 or int(np.prod(dims)) == 1                            # the nodes see the scene, not one constant
    md = np.abs(ADDRESS_HI - ADDRESS_LO)
    rng = np.random.default_rng(31)
    n = 4133
    pts = rng.uniform(ADDRESS_LO, ADDRESS_HI, (n, 3))
    out = np.arange(n) % 4 == 0                                                        # a quarter outside, on one to three axes, either side
    axes = rng.random((n, 3)) < 0.5
    axes[np.arange(n), rng.integers(0, 3, n)] = True
    shift = np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0) * (md * rng.uniform(0.0, 2.0, (n, 3)) + np.where(rng.random((n, 3)) < 0.5, 0.0, 1.0))
    beyond = np.where(shift < 0, ADDRESS_LO + shift, ADDRESS_HI + shift)
    pts = np.where(out[:, None] & axes, beyond, pts).astype(np.float32)
    inside = ((pts >= ADDRESS_LO) & (pts <= ADDRESS_HI)).all(-1)
    assert 0.2 < (~inside).mean() < 0.3
    cmg = _grid_only_cm(dict(dims=np.asarray(dims, np.int32), lim_min=ADDRESS_LO, map_dim=md, sdf=sdf, grad=grad))
    s, g = ops.sdf_points(cmg, _dev(pts), want_grad=True)
    c = grid_index(pts, ADDRESS_LO, md, dims)
    np.testing.assert_array_equal(s.cpu().numpy()[:, 0], sdf.cpu().numpy()[c[:, 0], c[:, 1], c[:, 2]])
    np.testing.assert_array_equal(g.cpu().numpy()[:, 0], grad.cpu().numpy()[c[:, 0], c[:, 1], c[:, 2]])


# ---------------------------------------------------------------------------------------------------------------------------
# part 4: a non-cubic grid recorded from the reference
# ---------------------------------------------------------------------------------------------------------------------------
def test_recorded_non_cubic_grid():
    """tests/golden/cost_grid3d_aniso.npz: this package's GridMapSDF reproduces the reference's cmap_dim, the precompute kernel the
    recorded grid (bounds of part 3), and GridMapSDF(X) on the recorded grid the recorded lookups and their gradients, array_equal."""
    import torch_robotics_amd as tra
    g = gold("cost_grid3d_aniso")
    lim, dims = g["limits"], g["cmap_dim"]
    objs = H.objects_from_golden(g, "fixed")
    assert len(objs) == 2 and all(np.abs(o["pos"]).max() > 0.1 and not np.allclose(o["R"], np.eye(3), atol=0.1) for o in objs)   # posed
    ta = dict(device=DEV, dtype=torch.float32)
    fields = [tra.ObjectField([tra.MultiSphereField(g["fixed0_f0_centers"], g["fixed0_f0_radii"], tensor_args=ta)], "posed_spheres",
                              pos=g["fixed0_pos"], ori=g["fixed0_ori"]),
              tra.ObjectField([tra.MultiBoxField(g["fixed1_f0_centers"], g["fixed1_f0_sizes"], tensor_args=ta)], "tilted_boxes",
                              pos=g["fixed1_pos"], ori=g["fixed1_ori"])]
    gm = tra.GridMapSDF(lim, float(g["cell"]), fields, tensor_args=ta)
    np.testing.assert_array_equal(gm.cmap_dim.cpu().numpy(), dims)
    orc = Oracle(model("panda_arm_no_gripper"), scene_only_spec(objs))
    nodes = linspace_nodes(dims, lim[0], lim[1])
    grid_precompute_check(gm.sdf_tensor.cpu().numpy(), gm.grad_sdf_tensor.cpu().numpy(), g["sdf"], g["grad"], nodes, orc, "GridMapSDF, recorded scene")
    sdf, grad = ops.grid_precompute(ops.CostHandle(scene_only_spec(objs), DEV), dims, lim[0], lim[1])
    grid_precompute_check(sdf.cpu().numpy(), grad.cpu().numpy(), g["sdf"], g["grad"], nodes, orc, "kernel, recorded scene")
    # the lookup on the RECORDED grid (the kernel's own differs from it in the last digits)
    gm.sdf_tensor, gm.grad_sdf_tensor, gm._qcm = _dev(g["sdf"]), _dev(g["grad"]), None
    X = _dev(g["pts"]).requires_grad_(True)
    val = gm(X)
    val.sum().backward()
    np.testing.assert_array_equal(val.detach().cpu().numpy(), g["pts_sdf"])
    np.testing.assert_array_equal(X.grad.cpu().numpy(), g["pts_grad"])
    inside = ((g["pts"] >= lim[0]) & (g["pts"] <= lim[1])).all(-1)
    assert 100 <= inside.sum() <= 400

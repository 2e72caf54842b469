"""Shared by tests/test_point3d_traj_cpu.py and tests/test_gpu_point3d_traj.py: the cases of the 3-D point mass's trajectory objective
(trk_point3d_traj_cost_grad, trk_point3d_traj_adam_steps), their seeded inputs and the fp64 reference of the objective:
Oracle.cost_fields on the one-column cost model + oracle.gp_factor_cost / oracle.gp_prior + the via term folded as include/trk.h states
it above TrkTrajVia."""
import numpy as np
import torch

import helpers as hp
from planar_traj_helpers import ADAM_ROUNDINGS, GROUPINGS, PARAMS, SHAPES, TOL_HINGE_COST, TOL_PRIOR_COST, TOL_PRIOR_GRAD  # noqa: F401
from torch_robotics_amd import _abi
from torch_robotics_amd.costmodel import CostModelSpec, grid_object, make_object, sphere_prims

FIELD_OBJECTS, FIELD_WS = _abi.FIELD_OBJECTS, _abi.FIELD_WS
# weights that are neither 0 nor 1: (w_obj, w_ws)
WEIGHTS = (0.7, 2.5)
# A clamped row is judged where the fp64 hinge of each field is decided by more than this: the fp32 distance of a point to a
# primitive of these scenes (coordinates below 2 m) carries a few 1e-7 m of rounding, the sphere ranking's near-tie rule a few 1e-6 m
# (trk_device.h, scene_min_sdf), so a margin - sdf within 1e-5 of zero may fall on either side of the relu in fp32.
CLAMP_BAND = 1e-5
# start spread of the walks around a primitive's centre, per scene (the issue's recipe: 0.15; widened or narrowed so that the clamped
# hinge is positive on at least 10 % of the pooled samples -- asserted in test_point3d_traj_cpu.py)
_cache = {}


def _scene_a():
    g = hp.gold("cost_spheres3d")
    return hp.objects_from_golden(g, "fixed"), None, g["limits"][0], g["limits"][1], np.float32(0.04), 0.15


def _scene_b():
    return hp.posed_scene_objects(), None, np.array([-0.8, -0.3, -1.4], np.float32), np.array([1.0, 1.4, 0.4], np.float32), np.float32(0.05), 0.15


def _scene_c():
    grid = hp.address_grid((5, 6, 7), hp.ADDRESS_LO, hp.ADDRESS_HI, seed=3, vlo=0.02, vhi=0.9, margin=hp.ADDRESS_MARGIN)
    c, r = hp.address_spheres(hp.ADDRESS_LO, hp.ADDRESS_HI)
    return [grid_object(), make_object(sphere_prims(c[:1], r[:1]))], grid, hp.ADDRESS_LO, hp.ADDRESS_HI, hp.ADDRESS_MARGIN, 0.15


SCENES = {"spheres": _scene_a, "posed": _scene_b, "grid": _scene_c}
CASES = [(name, clamp) for name in SCENES for clamp in (False, True)]


def spec_of(name, clamp) -> CostModelSpec:
    """the cost model of a scene for the point mass: one position column, which is the object-collision column, and the workspace box"""
    key = ("spec", name, bool(clamp))
    if key not in _cache:
        objects, grid, lo, hi, margin, _ = SCENES[name]()
        spec = CostModelSpec(n_links_in=1, objects=list(objects))
        spec.obj_link_idx = np.zeros(1, np.int32)
        spec.obj_link_margin = np.array([margin], np.float32)
        spec.grid = None if grid is None else dict(grid)
        spec.ws_min, spec.ws_max = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        spec.clamp_fields = (FIELD_OBJECTS | FIELD_WS) if clamp else 0
        spec.validate()
        _cache[key] = spec
    return _cache[key]


def primitive_centres(name):
    """world-frame centres (n, 3) fp64 of the analytic primitives of a scene"""
    out = []
    for o in SCENES[name]()[0]:
        for p in o["prims"]:
            out.append(o["pos"].astype(np.float64) + o["R"].astype(np.float64) @ np.asarray(p["center"], np.float64))
    return np.stack(out)


def walks(name, B, H):
    """(q, qd) (B, H, 3) fp32, seed 1000 B + H: start = the centre of a randomly chosen primitive + N(0, spread^2), increments
    N(0, 0.02^2), qd ~ N(0, 0.3^2); computed once and never written to"""
    key = ("walk", name, B, H)
    if key not in _cache:
        rng = np.random.default_rng(1000 * B + H)
        centres, spread = primitive_centres(name), SCENES[name]()[5]
        start = centres[rng.integers(len(centres), size=B)] + rng.standard_normal((B, 3)) * spread
        steps = np.concatenate([np.zeros((B, 1, 3)), np.cumsum(rng.standard_normal((B, H - 1, 3)) * 0.02, axis=1)], 1)
        q = (start[:, None, :] + steps).astype(np.float32)
        qd = (rng.standard_normal((B, H, 3)) * 0.3).astype(np.float32)
        q.setflags(write=False); qd.setflags(write=False)
        _cache[key] = (q, qd)
    return _cache[key]


def oracle_of(oracle, spec):
    """an Oracle on `spec` (the kinematic model is not used by cost_fields; the Panda stands in, as in tests/test_gpu_api.py)"""
    key = ("oracle", id(spec))
    if key not in _cache:
        if "model" not in _cache:
            _cache["model"] = hp.model("panda_arm_no_gripper")
        _cache[key] = (oracle.Oracle(_cache["model"], spec), spec)          # the spec is kept alive with its id
    return _cache[key][0]


def via_weights(n):
    """(alpha, beta) fp32 numpy, as ops.via_point_weights forms them"""
    alpha = torch.linspace(0, 1, int(n) + 2, dtype=torch.float32)[1:int(n) + 1]
    return alpha.numpy().copy(), (1 - alpha).numpy().copy()


def via_points(q, n):
    """(B, H-1, n, 3) fp32: q[b,t] * alpha[a] + q[b,t+1] * beta[a], each product and the sum rounded once in fp32"""
    alpha, beta = (w.reshape(1, 1, n, 1) for w in via_weights(n))
    q = np.asarray(q, np.float32)
    pts = (q[:, :-1, None, :] * alpha).astype(np.float32) + (q[:, 1:, None, :] * beta).astype(np.float32)
    assert pts.dtype == np.float32
    return pts


def hinge64(orc, pts, w_obj, w_ws):
    """fp64 weighted hinge at fp32 points (n, 3) -> (cost (n,), grad (n, 3), per-field values (n, 2) before the weights)"""
    p = np.asarray(pts).reshape(-1, 1, 3).astype(np.float64)
    co, go = orc.cost_fields(FIELD_OBJECTS, p, "f64")
    cw, gw = orc.cost_fields(FIELD_WS, p, "f64")
    return w_obj * co + w_ws * cw, (w_obj * go + w_ws * gw).reshape(-1, 3), np.stack([co, cw], -1)


def objective64(oracle, spec, q, qd, dt, sigma, gp_weight, w_obj, w_ws, via=None):
    """fp64 objective on fp32 inputs.  via: None or (w_via, n).
    -> dict(hinge (B,H), hinge_grad (B,H,3), fields (B,H,2), prior (B,H), prior_total (B,), prior_gq, prior_gqd, via_cost (B,H),
    via_grad (B,H,3), via_fields (B,H-1,n,2) or None, cost, gq, gqd)"""
    B, H, _ = q.shape
    orc = oracle_of(oracle, spec)
    c, g, f = hinge64(orc, q, w_obj, w_ws)
    c, g, f = c.reshape(B, H), g.reshape(B, H, 3), f.reshape(B, H, 2)
    q64, qd64 = np.asarray(q, np.float64), np.asarray(qd, np.float64)
    pf = oracle.gp_factor_cost(q64, qd64, dt, sigma, gp_weight, "f64")
    pt, pgq, pgqd = oracle.gp_prior(q64, qd64, dt, sigma, gp_weight, "f64")
    vc, vg, vf = np.zeros((B, H)), np.zeros((B, H, 3)), None
    if via is not None and H > 1:
        w_via, n = via
        alpha, beta = (w.astype(np.float64).reshape(1, 1, n, 1) for w in via_weights(n))
        hv, gv, fv = hinge64(orc, via_points(q, n), w_obj, w_ws)
        hv, gv, vf = hv.reshape(B, H - 1, n), gv.reshape(B, H - 1, n, 3), fv.reshape(B, H - 1, n, 2)
        vc[:, :H - 1] = w_via * hv.sum(-1)
        vg[:, :H - 1] += w_via * (alpha * gv).sum(2)
        vg[:, 1:] += w_via * (beta * gv).sum(2)
    return dict(hinge=c, hinge_grad=g, fields=f, prior=pf, prior_total=pt, prior_gq=pgq, prior_gqd=pgqd, via_cost=vc, via_grad=vg,
                via_fields=vf, cost=c + vc + pf, gq=g + vg + pgq, gqd=pgqd)


def cost_bound(ref):
    """the sum of the hinge's (way points and via points) and the prior's cost bounds, each on the batch's scale"""
    return TOL_HINGE_COST * (np.abs(ref["hinge"]).max() + np.abs(ref["via_cost"]).max()) + TOL_PRIOR_COST * np.abs(ref["prior"]).max()


def raw_fields(oracle, name, pts):
    """(n, 2) fp64: margin - sdf of the object field and of the workspace box at fp32 points, WITHOUT the clamp"""
    return hinge64(oracle_of(oracle, spec_of(name, False)), pts, 1.0, 1.0)[2]


def decided(fields, band=CLAMP_BAND):
    """rows whose per-field fp64 values (..., 2) = margin - sdf (unclamped) all lie more than `band` from the relu's corner"""
    return (np.abs(fields) > band).all(-1)


def off_faces(name, pts, band=hp.FACE_BAND):
    """rows of fp32 points (n, 3) at least `band` from every cell face of the scene's voxel grid (all rows without a grid): there the
    fp32 kernel and the fp64 oracle read the same cell -- the grid's distance is piecewise constant, so a point on a face has two costs"""
    grid = SCENES[name]()[1]
    p = np.asarray(pts, np.float64).reshape(-1, 1, 3)
    return np.ones(len(p), bool) if grid is None else hp.off_face_rows(p, grid, band)


def pin_masks(pin, B, H):
    """boolean (B, H, 6) over (q, qd): the components the mask `pin` holds"""
    m = np.zeros((B, H, 6), bool)
    if pin & 1: m[:, 0, :3] = True
    if pin & 2: m[:, H - 1, :3] = True
    if pin & 4: m[:, 0, 3:] = True
    if pin & 8: m[:, H - 1, 3:] = True
    return m

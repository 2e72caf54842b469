"""Shared by tests/test_planar_traj_cpu.py and tests/test_gpu_planar_traj.py: the cases of the 2-D point mass's trajectory objective
(trk_scene2d_traj_cost_grad, trk_scene2d_traj_adam_steps), their seeded inputs and the fp64 reference of the objective,
w_obj x helpers.planar64 + oracle.gp_factor_cost / oracle.gp_prior."""
import numpy as np

import helpers as hp

# (fixture, grid, analytic, workspace): grid + analytic + workspace, analytic + workspace, the thin grid + workspace
SCENES = [("gridposed", True, True, True), ("posed", False, True, True), ("gridthin", True, False, True)]
# (dt, sigma, gp_weight, w_obj)
PARAMS = [(0.08, 1.0, 1.0, 20.0), (5.0 / 64, 0.5, 0.3, 1.0)]
# one lane; the wavefront edge on both sides; a trajectory over two and four wavefronts; several trajectories per workgroup with a ragged
# last workgroup ((5,63): 4 per workgroup, (37,64): 4 per workgroup and 10 workgroups, (3,3): 85 per workgroup); the upper limit
SHAPES = [(1, 1), (1, 2), (3, 3), (5, 63), (4, 64), (3, 65), (2, 128), (7, 200), (2, 256), (37, 64)]
GROUPINGS = (1, 2, 31, 32, 33, 70)
TOL_HINGE_COST, TOL_PRIOR_COST, TOL_PRIOR_GRAD = 1e-5, 2e-5, 1e-4      # tests/test_gpu_planar2d_edges.py, test_gp_prior_vs_fp64_oracle

# fp32 roundings between the returned (m, v) and the stored x on the kernel's update path (adam_component in csrc/trk_planar.hip):
# lr / bc1, sqrtf(v1), the fma sqrt * rsqrt_bc2 + eps, the fp32 value of eps = 1e-8, m1 / denom, step * quotient.  The final
# subtraction is the half ulp of the stored value.
ADAM_ROUNDINGS = 6


def random_walks(limits, B, H, seed):
    """(q, qd) (B, H, 2) fp32: starts uniform in the scene limits, increments N(0, 0.05^2) -- some walks leave the workspace --,
    qd ~ N(0, 0.3^2)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(limits, np.float64)
    q = rng.uniform(lo, hi, (B, 1, 2)) + np.concatenate([np.zeros((B, 1, 2)), np.cumsum(rng.standard_normal((B, H - 1, 2)) * 0.05, axis=1)], 1)
    return q.astype(np.float32), (rng.standard_normal((B, H, 2)) * 0.3).astype(np.float32)


def objective64(oracle, a, q, qd, dt, sigma, gp_weight, w_obj, clamp):
    """fp64 objective on fp32 inputs.  a: dict(objects, margin, ws, grid) as helpers.planar64 takes them.
    -> dict(hinge (B,H), hinge_grad (B,H,2), sdf (n, n_df), prior (B,H), prior_total (B,), prior_gq, prior_gqd, cost, gq, gqd)"""
    B, H, _ = q.shape
    c, g, sdf, _ = hp.planar64(a["objects"], q.reshape(-1, 2), a["margin"], ws=a["ws"], grid=a["grid"], clamp=clamp)
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    pf = oracle.gp_factor_cost(q64, qd64, dt, sigma, gp_weight, "f64")
    pt, pgq, pgqd = oracle.gp_prior(q64, qd64, dt, sigma, gp_weight, "f64")
    c, g = c.reshape(B, H), g.reshape(B, H, 2)
    return dict(hinge=c, hinge_grad=g, sdf=sdf, prior=pf, prior_total=pt, prior_gq=pgq, prior_gqd=pgqd,
                cost=w_obj * c + pf, gq=w_obj * g + pgq, gqd=pgqd)


def cost_bound(ref, w_obj):
    """the sum of the hinge's and the prior's cost bounds, each on the batch's scale"""
    return TOL_HINGE_COST * abs(w_obj) * np.abs(ref["hinge"]).max() + TOL_PRIOR_COST * np.abs(ref["prior"]).max()


def pin_masks(pin, B, H):
    """boolean (B, H, 4) over (q.x, q.y, qd.x, qd.y): the components the mask `pin` holds"""
    m = np.zeros((B, H, 4), bool)
    if pin & 1: m[:, 0, :2] = True
    if pin & 2: m[:, H - 1, :2] = True
    if pin & 4: m[:, 0, 2:] = True
    if pin & 8: m[:, H - 1, 2:] = True
    return m

"""Collision and joint-limit decisions at their edges, far from the world origin, per sample against the fp64 oracle.

The equal-radius sphere path ranks spheres by a key that cancels a squared distance (scene_min_sdf), and the fast boolean path
forms d^2 from the same keys (spec_collision_links).  Both used to cancel |p|^2 about the WORLD origin, so their error grew with
the distance of robot and scene from it (a wrong sphere 4.5e-5 m off a near-tie at 3 m).  Here every point is checked on its own,
not as a whole-tensor ratio or a mismatch fraction, and every check also asserts that enough points really fall into the hard
regions (near-ties, near-threshold) so that it cannot quietly become a no-op.

Bounds (per point, metres):
  - S_BOUND_RANKED: the equal-radius ranking picks a sphere whose distance is within this of the nearest one's (the masked index
    bits and the key's rounding are ~2^-19 of a scene-sized square); the same at 30 m as at the origin;
  - S_BOUND_EXACT: the per-sphere path (mixed radii, the control) and any correctly ranked winner: the fp32 distance itself;
  - booleans equal the fp64 decision wherever the fp64 distance lies more than BAND_ULPS ulp of the threshold from it;
  - gradients are the fp64 winner's unit vector (or the runner-up's where that one lies within S_BOUND_RANKED).
"""
import numpy as np
import pytest
import torch

from helpers import gold, model
from oracle.oracle import Oracle
from torch_robotics_amd import ops
from torch_robotics_amd._abi import FIELD_OBJECTS
from torch_robotics_amd.costmodel import CostModelSpec, box_prims, make_object, sphere_prims

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MG = np.float32(0.1)                   # margin of every collision link
R_EQ = np.float32(0.05)                # radius of the equal-radius scenes
S_BOUND_RANKED = 5e-6
S_BOUND_EXACT = 1e-6
BAND_ULPS = 8
GRAD_TOL = 1e-5
OFFSETS = [(0.0, 0.0, 0.0), (1.0, 0.3, 0.2), (3.0, 1.0, 0.5), (10.0, 3.0, 2.0), (30.0, -20.0, 1.0)]
TIE_GAPS = [1e-7, 1e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3]
THR_ULPS = [0, 1, 4, 16, 64, 256]
THR_ABS = [1e-6, 4e-6, 1.6e-5]


def _rot(seed):
    a = np.random.default_rng(seed).standard_normal(4)
    w, x, y, z = a / np.linalg.norm(a)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _centres(rng, n, min_sep=0.16, half=0.5):
    c = []
    while len(c) < n:
        p = rng.uniform(-half, half, 3)
        if all(np.linalg.norm(p - q) > min_sep for q in c):
            c.append(p)
    return np.array(c)


def _scene(kind, seed=0):
    """(centres (n, 3) fp64, radii (n,), box (centre, size) or None) in the scene's own frame"""
    rng = np.random.default_rng(seed)
    n = {"fast": 12, "box": 12, "many": 20, "mixed": 12}[kind]
    c = _centres(rng, n)
    r = np.full(n, float(R_EQ)) if kind != "mixed" else rng.uniform(0.03, 0.08, n).astype(np.float32).astype(np.float64)
    box = (np.array([0.9, 0.9, 0.9]), np.array([0.2, 0.3, 0.25])) if kind == "box" else None
    return c, r, box


def _place(c_loc, box, O, R):
    """world-frame sphere centres, rounded to fp32 once (the scene is given in world coordinates), and the box object"""
    cw = (c_loc @ R.T + np.asarray(O)).astype(np.float32)
    bobj = None
    if box is not None:
        bobj = make_object(box_prims(np.zeros((1, 3)), box[1][None, :], rounded=True), (R @ box[0] + np.asarray(O)).astype(np.float32),
                           R.astype(np.float32))
    return cw, bobj


def _spec(cw, r, bobj):
    g = gold("panda_robot")
    K = len(g["obj_link_idxs"])
    spec = CostModelSpec(n_links_in=11)
    spec.obj_link_idx = g["obj_link_idxs"]
    spec.obj_link_margin = np.full(K, MG, np.float32)
    spec.objects = [make_object(sphere_prims(cw, r.astype(np.float32)))] + ([bobj] if bobj is not None else [])
    spec.validate()
    return spec, K


def _sphere_dists(p, cw, r):
    """fp64 signed distances (n, n_spheres) of fp32 points to the fp32 spheres"""
    d = np.linalg.norm(p[:, None, :].astype(np.float64) - cw[None].astype(np.float64), axis=-1)
    return d - r.astype(np.float32).astype(np.float64)[None]


def _points(c, r, rng):
    """points in the scene frame (fp64): near-ties of two spheres and near-threshold points of one, no third sphere close"""
    n = len(c)
    ties, thr = [], []
    for gap in TIE_GAPS:
        made = 0
        while made < 40:
            a, b = rng.choice(n, 2, replace=False)
            if np.linalg.norm(c[a] - c[b]) > 0.5:
                continue
            ab = c[b] - c[a]
            L = np.linalg.norm(ab)
            e = ab / L
            u = rng.standard_normal(3)
            u -= u.dot(e) * e
            u /= np.linalg.norm(u)
            dd = rng.uniform(0.12, 0.3) + r[a]                        # centre distance of the nearer sphere, about
            h2 = dd * dd - (L / 2) ** 2
            if h2 <= 1e-4:
                continue
            # surface distances s_a < s_b with (s_b - s_a) = gap * s_a: move off the bisector towards a
            mid = c[a] + 0.5 * ab + np.sqrt(h2) * u
            sa = np.linalg.norm(mid - c[a]) - r[a]
            target = gap * max(sa, 1e-3)
            # d|p - c_b| - d|p - c_a| along -e is about 2 * (L / 2) / dd per metre
            t = target / (L / dd)
            p = mid - t * e
            ds = np.linalg.norm(c - p, axis=1) - r
            o = np.argsort(ds)
            if o[0] != a or o[1] != b or ds[o[2]] < ds[a] + 0.02:
                continue
            ties.append(p)
            made += 1
    for k in range(n):
        for off in [s * u * 1e-9 for u in THR_ULPS for s in (1, -1)] + [s * a for a in THR_ABS for s in (1, -1)]:
            for _ in range(2):
                u = rng.standard_normal(3)
                u /= np.linalg.norm(u)
                T = float(np.float32(MG + np.float32(r[k])))
                off_m = off if abs(off) >= 1e-6 else off / 1e-9 * float(np.spacing(np.float32(T)))
                p = c[k] + u * (T + off_m)
                ds = np.linalg.norm(c - p, axis=1) - r
                if np.argmin(ds) == k and np.partition(ds, 1)[1] > ds[k] + 0.02:
                    thr.append(p)
    return np.array(ties), np.array(thr)


def _box_sdf_far(p, bobj, margin=0.05):
    """points the box is not nearest to by at least `margin` (conservative: distance to its bounding sphere)"""
    if bobj is None:
        return np.full(len(p), np.inf)
    return np.linalg.norm(p - bobj["pos"].astype(np.float64), axis=1) - 0.3


@pytest.mark.parametrize("kind", ["fast", "box", "many", "mixed"])
def test_scene_fields_far_from_origin(kind):
    """collision_fields / cost_fields on given positions, generated and table-driven, for scenes at 0 .. 36 m from the origin"""
    c, r, box = _scene(kind)
    rng = np.random.default_rng(7)
    ties_loc, thr_loc = _points(c, r, rng)
    bound = S_BOUND_EXACT if kind == "mixed" else S_BOUND_RANKED
    worst = {}
    cases = [(O, np.eye(3)) for O in OFFSETS] + [(OFFSETS[-1], _rot(3))]
    for O, R in cases:
        cw, bobj = _place(c, box, O, R)
        spec, K = _spec(cw, r, bobj)
        cm = ops.CostHandle(spec, DEV)
        orc = Oracle(model("panda_arm_no_gripper"), spec)
        pts = (np.concatenate([ties_loc, thr_loc]) @ R.T + np.asarray(O)).astype(np.float32)
        n_ties = len(ties_loc)
        d = _sphere_dists(pts, cw, r)
        order = np.argsort(d, axis=1)
        d1, d2 = np.take_along_axis(d, order[:, :1], 1)[:, 0], np.take_along_axis(d, order[:, 1:2], 1)[:, 0]
        assert (_box_sdf_far(pts.astype(np.float64), bobj) > d1 + 0.05).all()
        pos = np.repeat(pts[:, None, :], 11, axis=1)
        c64, _ = orc.cost_fields(FIELD_OBJECTS, pos.astype(np.float64), prec="f64")
        s64 = (K * float(MG) - c64) / K
        assert np.abs(s64 - d1).max() < 1e-12                         # the oracle's minimum is the nearest sphere's
        b64 = orc.collision_fields(FIELD_OBJECTS, pos.astype(np.float64), prec="f64")
        thr64 = float(MG) + r[order[:, 0]].astype(np.float32).astype(np.float64)
        band = BAND_ULPS * np.spacing(thr64.astype(np.float32)).astype(np.float64)
        decided = np.abs(s64 - float(MG)) > band
        # coverage: near-ties where a wrong sphere would be seen, near-threshold points on both sides inside the fast path's old band
        gap = d2 - d1
        if kind != "mixed":
            assert ((gap[:n_ties] > bound) & (gap[:n_ties] < 1e-4)).sum() >= 40, (O, kind)
            assert (gap[:n_ties] < bound).sum() >= 40, (O, kind)
        near = s64[n_ties:] - float(MG)
        assert ((near > 0) & (near < 2e-5) & decided[n_ties:]).sum() >= 20 and ((near < 0) & (near > -2e-5) & decided[n_ties:]).sum() >= 20
        pt = torch.as_tensor(pos, device=DEV)
        for generated in (True, False):
            cm.enable_specialized(generated)
            what = f"{kind} O={O} rotated={not np.array_equal(R, np.eye(3))} generated={generated}"
            hit = ops.collision_fields(cm, FIELD_OBJECTS, pt).cpu().numpy()
            cost, g = ops.cost_fields(cm, FIELD_OBJECTS, pt, want_grad=True)
            torch.cuda.synchronize()
            s = (K * float(MG) - cost.cpu().numpy().astype(np.float64)) / K
            err = np.abs(s - s64)
            worst[what] = float(err.max())
            bad = np.flatnonzero(err > bound)
            assert len(bad) == 0, (f"{what}: {len(bad)} points off by more than {bound:g} m, worst {err.max():.3g} m "
                                   f"(fp64 runner-up gap there {gap[np.argmax(err)]:.3g} m)")
            wrong = np.flatnonzero((hit != b64) & decided)
            assert len(wrong) == 0, (f"{what}: {len(wrong)} booleans differ from fp64 outside the {BAND_ULPS}-ulp band; "
                                     f"worst |d - thr| {np.abs(s64[wrong] - float(MG)).max():.3g} m")
            # gradient of every collision link column: minus the unit vector from the winning centre
            gl = g.cpu().numpy().astype(np.float64)[:, spec.obj_link_idx, :]
            p64 = pts.astype(np.float64)
            def unit(j):
                v = p64 - cw[j].astype(np.float64)
                return -v / np.linalg.norm(v, axis=1, keepdims=True)
            e1 = np.abs(gl - unit(order[:, 0])[:, None, :]).max(axis=(1, 2))
            e2 = np.abs(gl - unit(order[:, 1])[:, None, :]).max(axis=(1, 2))
            ok = (e1 < GRAD_TOL) | ((e2 < GRAD_TOL) & (gap <= bound))
            assert ok.all(), f"{what}: {int((~ok).sum())} gradients are neither the fp64 winner's nor a tied runner-up's"
        cm.enable_specialized(True)
    print({k: f"{v:.3g}" for k, v in worst.items()})


def _panda_limits(m):
    lo, hi = np.asarray(m.lower[m.dof_idx >= 0], np.float32), np.asarray(m.upper[m.dof_idx >= 0], np.float32)
    o = np.argsort(m.dof_idx[m.dof_idx >= 0])
    return lo[o], hi[o]


@pytest.mark.parametrize("T,H,n_interp", [(147, 3, 4), (49, 9, 10)])
def test_via_limit_flags_at_the_limits(T, H, n_interp):
    """Fused joint-limit flags of rollout_collision_via on way points exactly on a limit, one ulp either side, signed zeros on a zero
    limit, +-inf and NaN, in the first, a middle and the last way point: equal to the three-launch flags and to (x >= lo) & (x <= hi).
    (147, 3, 4): eight interpolated configurations per trajectory, several trajectories per wavefront; (49, 9, 10): 80, one trajectory
    over two wavefronts."""
    m = model("panda_arm_no_gripper")
    h = ops.ModelHandle(m)
    spec = CostModelSpec(n_links_in=11)
    g = gold("panda_robot")
    spec.obj_link_idx, spec.obj_link_margin = g["obj_link_idxs"], np.full(len(g["obj_link_idxs"]), MG, np.float32)
    spec.objects = [make_object(sphere_prims(np.array([[5.0, 5.0, 5.0]]), np.float32(0.05)))]     # nothing collides
    spec.validate()
    cm = ops.CostHandle(spec, DEV)
    lo, hi = _panda_limits(m)
    # joint 0 gets a zero lower limit, joint 1 a zero upper limit (as signed zeros of the other sign), the rest keep the URDF's
    lo, hi = lo.copy(), hi.copy()
    lo[0], hi[1] = np.float32(0.0), np.float32(-0.0)
    lo_t, hi_t = torch.as_tensor(lo, device=DEV), torch.as_tensor(hi, device=DEV)
    mid = (0.5 * (lo + hi)).astype(np.float32)
    mid[0], mid[1] = np.float32(0.5), np.float32(-0.5)
    # (joint, value): signed zeros on the zero limits, +-inf, NaN, then every limit exactly and one ulp either side
    edges = [(0, np.float32(-0.0)), (0, np.float32(0.0)), (1, np.float32(0.0)), (1, np.float32(-0.0)),
             (2, np.float32(np.inf)), (3, np.float32(-np.inf)), (4, np.float32(np.nan))]
    for j in range(7):
        for v in (lo[j], hi[j]):
            edges += [(j, v), (j, np.nextafter(v, np.float32(np.inf))), (j, np.nextafter(v, np.float32(-np.inf)))]
    assert T >= len(edges)
    x = np.tile(mid, (T, H, 1)).astype(np.float32)
    for t in range(T):                                            # one edge value per trajectory, in turn in the first, a middle, the last way point
        j, v = edges[t % len(edges)]
        x[t, (0, H // 2, H - 1)[(t // len(edges) + t) % 3], j] = v
    with np.errstate(invalid="ignore"):
        inside = ((x >= lo) & (x <= hi)).all(axis=(1, 2))
    assert (~inside).sum() >= T // 4 and inside.sum() >= T // 4      # both outcomes occur
    xt = torch.as_tensor(x, device=DEV)
    wp, buf = ops.rollout_collision_via(h, cm, FIELD_OBJECTS, xt, n_interp, margin=0.0, limits=(lo_t, hi_t))
    fused = ops.traj_validate(None, xt, 7, lo_t, hi_t, flags=buf).flags.cpu().numpy()
    three = ops.traj_validate(wp, xt, 7, lo_t, hi_t).flags.cpu().numpy()
    expect = np.where(inside, 0, 2).astype(np.uint8)
    assert np.array_equal(three, expect), np.flatnonzero(three != expect)
    bad = np.flatnonzero(fused != expect)
    assert len(bad) == 0, f"fused flags differ at trajectories {bad.tolist()}: way points {[x[t][~np.isclose(x[t], mid)].tolist() for t in bad[:4]]}"


def _spheres16(rng, O):
    """a dense 16-sphere scene in the Panda's reach, moved by O (world coordinates, fp32)"""
    c = []
    while len(c) < 16:
        p = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.0])
        if np.linalg.norm(p[:2]) > 0.25 and all(np.linalg.norm(p - q) > 0.12 for q in c):
            c.append(p)
    return (np.array(c) + np.asarray(O)).astype(np.float32)


@pytest.mark.parametrize("O", [(0.0, 0.0, 0.0), (3.0, 1.0, 0.5), (10.0, 3.0, 2.0)])
def test_fused_rollout_collision_far_from_origin(O):
    """rollout_collision with the Panda's base and a dense 16-sphere scene moved together: per-sample booleans against fp64 distances
    of the fp64 link positions, outside the FK bound + band"""
    m = model("panda_arm_no_gripper")
    h = ops.ModelHandle(m)
    h.set_base_pose(np.eye(3, dtype=np.float32), np.asarray(O, np.float32))
    rng = np.random.default_rng(11)
    cw = _spheres16(rng, O)
    r = np.full(16, R_EQ, np.float32)
    spec, K = _spec(cw, r, None)
    cm = ops.CostHandle(spec, DEV)
    lo, hi = _panda_limits(m)
    n = 65536
    q = rng.uniform(lo, hi, (n, 7)).astype(np.float32)
    hit = ops.rollout_collision(h, cm, FIELD_OBJECTS, torch.as_tensor(q, device=DEV)).cpu().numpy()
    assert ops.last_dispatch() == "generated"
    # the base is a pure translation: the fp64 world positions are the chain's (the position columns of the rollout) plus O, exactly
    pos64, _, _ = Oracle(m, spec).rollout(q.astype(np.float64), (0, 1, 0, 0), "f64")
    pl = pos64[:, spec.obj_link_idx, :] + np.asarray(O, np.float32).astype(np.float64)
    d = _sphere_dists(pl.reshape(-1, 3), cw, r).reshape(n, K, 16)
    ds = np.sort(d, axis=-1)
    s64 = ds[..., 0]
    fk = 2e-6 * max(1.0, float(np.abs(pl).max()))
    decided = (np.abs(s64 - float(MG)) > fk + BAND_ULPS * 1.5e-8).all(axis=1)
    b64 = (s64 < float(MG)).any(axis=1)
    tied = ((ds[..., 1] - ds[..., 0]) < 1e-4 * np.abs(ds[..., 0]) + 1e-9).any(axis=1)
    assert tied.sum() >= 4, tied.sum()
    assert ((np.abs(s64 - float(MG)) < 1e-4).any(axis=1)).sum() >= 50
    wrong = np.flatnonzero((hit != b64) & decided)
    assert len(wrong) == 0, f"O={O}: {len(wrong)} booleans differ from fp64 outside the FK bound + band"
    # the fused cost (FAST instantiation): per sample within K x (FK bound x hinge slope 1 + the ranking bound)
    _, cost, _ = ops.rollout_cost_grad(h, cm, (0, 1, 0, 0), torch.as_tensor(q, device=DEV))
    assert ops.last_dispatch() == "generated"
    c64 = (K * float(MG) - s64.sum(axis=1))
    err = np.abs(cost.cpu().numpy().astype(np.float64) - c64)
    assert err.max() <= K * (fk + S_BOUND_RANKED), f"O={O}: worst per-sample cost error {err.max():.3g}"


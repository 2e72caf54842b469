"""The fused boolean path of the attached-point models (k_pcoll; ops.rollout_points_collision, ops.rollout_points_collision_via and
the task routing on top of them): the Panda with the 45 link spheres, with the grasped box, with both -- on EnvSpheres3D, on
EnvTableShelf and (the grasped box) on a voxel grid.

References: the reference's own booleans (grasp_panda.npz), the fp64 oracle (Oracle.fk_points + Oracle.collision_fields) and the
two-step path the fused kernel replaces (fk_points + collision_fields; the via points materialised first), which is also the task's
routing under TRK_POINTS_COLLISION_FUSED=0.

fp64 oracle, override margins m: a sample is UNSTABLE when the oracle's answer differs between m - 1e-5 and m + 1e-5.  The band is
5 x TOL_H (TOL_H = 2e-6: the bound every FK test of this suite holds fp32 positions to) and a signed distance is 1-Lipschitz in the
point's position, so a stable sample's decision cannot depend on fp32 rounding: it must equal the oracle's byte.  On the voxel grid
the distance is piecewise constant, not Lipschitz: there a sample also counts as unstable when one of its points lies within
helpers.FACE_BAND of a cell face (helpers.off_face_rows), where fp32 and fp64 may read neighbouring cells, or in a cell whose stored
value lies within the band of the margin (Case.oracle).  The margin-unstable share must stay below 0.5 % (it is at most 2 of 4133
samples for every model, analytic scene and mask, oracle alone; on the grid: of the samples the table does not decide) and the
near-face share below twice its geometric expectation (Case.__init__), so the check cannot thin itself out.
Self-collision alone hits 0 - 1 % of uniform samples at the margins 0.0 / 0.07; its mask is also run at SELF_MARGIN = 0.15, where
the oracle alone finds 1.8 % (spheres) and 4.2 % (box models) of the 4133 samples in collision
(tests/test_points_collision_cpu.py::test_self_margin_of_the_gpu_tests_gives_both_outcomes)."""
import copy
import os

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
from helpers import FACE_BAND, gold, grasp_panda_setup, grid_index, off_face_rows
from torch_robotics_amd import _abi, ops
from torch_robotics_amd._abi import FIELD_OBJECTS, FIELD_SELF, FIELD_WS
from torch_robotics_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TA = dict(device=DEV, dtype=torch.float32)
ALLF = FIELD_SELF | FIELD_OBJECTS | FIELD_WS
MASKS = (FIELD_SELF, FIELD_OBJECTS, FIELD_WS, FIELD_OBJECTS | FIELD_WS, ALLF)
NS = (1, 63, 65, 1000, 4133)
N_ALL = NS[-1]
BAND = 1e-5                     # 5 x TOL_H
SELF_MARGIN = 0.15
MAX_UNSTABLE_SHARE = 0.005
MOVED_BASE = [0.1234, -0.2345, 0.0567, 0.9659258, 0.0, 0.0, 0.2588190]       # xyz + wxyz, as KinModel.set_base_pose

ROBOTS = {
    "spheres": lambda: tra.RobotPanda(link_sphere_model="panda", tensor_args=TA),
    "grasp": lambda: tra.RobotPanda(grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
    "both": lambda: tra.RobotPanda(link_sphere_model="panda", grasped_object=tra.GraspedObjectPandaBox(tensor_args=TA), tensor_args=TA),
}
ENVS = {
    "spheres3d": lambda: tra.EnvSpheres3D(tensor_args=TA),
    "table_shelf": lambda: tra.EnvTableShelf(tensor_args=TA),
    # 21 cells per axis: no cell face through the coordinates the model holds constant (x = y = 0, z = 0.333 of the first links)
    "grid": lambda: tra.EnvSpheres3D(tensor_args=TA, precompute_sdf_obj_fixed=True, sdf_cell_size=0.096),
}
CASES = [(r, e) for e in ("spheres3d", "table_shelf") for r in ROBOTS] + [("grasp", "grid")]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def margins_of(fl):
    return (None, 0.0, 0.07) + ((SELF_MARGIN,) if fl == FIELD_SELF else ())


def _host_spec(spec):
    """the spec with the voxel grid's tables as host arrays (the oracle reads them on the CPU)"""
    if getattr(spec, "grid", None) is None:
        return spec
    host = copy.copy(spec)
    host.grid = {k: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in spec.grid.items()}
    return host


class Case:
    """One model on one scene: task, handles, the 4133 uniform configurations, their fp64 point positions and the oracle's bytes
    (computed once per mask and margin, shared by every test of the case)."""

    def __init__(self, robot_name, env_name, oracle_lib):
        self.robot = ROBOTS[robot_name]()
        self.task = tra.PlanningTask(env=ENVS[env_name](), robot=self.robot, obstacle_cutoff_margin=0.03, tensor_args=TA)
        self.spec = self.task.build_cost_spec()
        self.pl, self.po = self.robot.collision_point_set()
        self.kin = self.robot.diff_panda._kin
        self.oracle_lib = oracle_lib
        self.orc = oracle_lib.Oracle(self.kin, _host_spec(self.spec))
        self.model, self.cm = self.task._fused_handles(DEV)
        self.ps = self.robot._point_set(DEV)
        assert self.ps.specialized
        self.q_min, self.q_max = self.robot.q_min_np.astype(np.float64), self.robot.q_max_np.astype(np.float64)
        self.q_np = np.random.default_rng(11).uniform(self.q_min, self.q_max, (N_ALL, 7)).astype(np.float32)
        self.q = dev(self.q_np)
        self.pos64 = self.orc.fk_points(self.pl, self.po, self.q_np.astype(np.float64), "f64")
        grid = self.grid = getattr(self.orc.spec, "grid", None)
        tested = [int(i) for i in self.spec.obj_link_idx]          # the columns that are looked up in the grid
        self.off_face = off_face_rows(self.pos64[:, tested], grid, FACE_BAND) if grid is not None else np.ones(N_ALL, bool)
        if grid is not None:
            # the share of samples near a face is geometry, not rounding: 2 FACE_BAND / cell per coordinate, 3 coordinates of each
            # tested column (1.2 % for the 19 columns of the grasped-box model at 21 cells over 2 m); held to twice that
            assert tuple(int(v) for v in grid["dims"]) == (21, 21, 21)
            expect = 3 * len(tested) * 2 * FACE_BAND / (2.0 / 21)
            assert (~self.off_face).mean() <= 2 * expect, (int((~self.off_face).sum()), expect)
            # the stored distance of the cell of every tested point (Case.oracle)
            cell = grid_index(self.pos64[:, tested].astype(np.float32).reshape(-1, 3), grid["lim_min"], grid["map_dim"], grid["dims"])
            self.stored = np.asarray(grid["sdf"], np.float32)[cell[:, 0], cell[:, 1], cell[:, 2]].reshape(N_ALL, len(tested))
        self._bytes = {}

    def oracle(self, fl, margin):
        """(the oracle's bytes, stable rows) for an override margin"""
        key = (fl, margin)
        if key not in self._bytes:
            f = lambda m: self.orc.collision_fields(fl, self.pos64, m, "f64").astype(bool)
            stable = f(margin - BAND) == f(margin + BAND)
            # The 0.5 % condition -- with one exception, stated exactly.  The voxel grid's distance is piecewise constant: a sample is
            # margin-unstable there exactly when a tested point sits in a cell whose STORED value lies within the band of the margin,
            # whatever the arithmetic (at margin 0.0: 30 of the 9261 cells, 6.5 % of the samples).  Those samples are found in the
            # table itself (self.stored) and left out on the grid scene only; every other unstable sample counts towards the 0.5 %.
            ties = np.zeros(N_ALL, bool)
            if self.grid is not None and (fl & FIELD_OBJECTS):
                ties = (np.abs(self.stored.astype(np.float64) - margin) <= BAND * (1 + 1e-6)).any(1)
            print(f"unstable: mask {fl} margin {margin}: {int((~stable).sum())} of {N_ALL}, of them {int((~stable & ties).sum())} with a stored "
                  f"cell value within the band ({int(ties.sum())} samples touch such a cell)")
            assert (~stable & ~ties & self.off_face).mean() <= MAX_UNSTABLE_SHARE, (fl, margin, int((~stable & ~ties).sum()))
            assert ties.mean() <= 0.15, (fl, margin, int(ties.sum()))         # 537 of 4133 at margin 0.0, none at 0.07
            if margin != 0.0:
                assert (~stable).mean() <= MAX_UNSTABLE_SHARE, (fl, margin, int((~stable).sum()))
            self._bytes[key] = (f(margin), stable & self.off_face)
        return self._bytes[key]


_cases = {}


@pytest.fixture
def case(request, oracle_lib):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(*key, oracle_lib)
    return _cases[key]


def _raw_collision(ps, cm, fl, q, margin, out):
    """the C entry point on a caller's output buffer (for the sentinel bytes around it)"""
    B, Hh = (q.shape[0], q.shape[1]) if q.dim() == 3 else (q.shape[0], 1)
    m = float("nan") if margin is None else float(margin)
    with torch.cuda.device(DEV):
        rc = lib().trk_rollout_points_collision(ps._h, cm._h, fl, q.data_ptr(), B, Hh, m, out.data_ptr(), None,
                                                torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == _abi.TRK_OK, lib().trk_last_error()


def test_reference_goldens_of_the_grasped_box():
    """grasp_panda.npz: the reference's booleans per field, with the fields' own margins and with margin 0 -- exactly."""
    g = gold("grasp_panda")
    m, pl, po, spec = grasp_panda_setup()
    h = ops.ModelHandle(m)
    ps, cm = ops.PointSetHandle(h, pl, po, DEV), ops.CostHandle(spec, DEV)
    q = dev(g["q"])                                             # (4, 8, 7)
    for name, fl in (("self", FIELD_SELF), ("obj", FIELD_OBJECTS), ("ws", FIELD_WS)):
        got = ops.rollout_points_collision(ps, cm, fl, q)
        assert ops.last_dispatch() == "generated"
        assert got.shape == (4, 8) and got.dtype == torch.bool
        np.testing.assert_array_equal(got.cpu().numpy(), g[f"coll_{name}"], err_msg=name)
        np.testing.assert_array_equal(ops.rollout_points_collision(ps, cm, fl, q, margin=0.0).cpu().numpy(), g[f"coll0_{name}"], err_msg=name)
    total = g["coll_self"] | g["coll_obj"] | g["coll_ws"]
    np.testing.assert_array_equal(ops.rollout_points_collision(ps, cm, ALLF, q).cpu().numpy(), total)


@pytest.mark.parametrize("case", CASES, indirect=True, ids=lambda c: f"{c[0]}-{c[1]}")
def test_fused_vs_oracle_and_two_step(case):
    """Every mask, margin and batch size: against the two-step path byte for byte (at most max(1, n // 2000) bytes may differ -- the
    bound of test_fused_collision_vs_golden_and_two_step -- and, for an override margin, only on unstable samples), and every stable
    sample against the fp64 oracle.  Sentinel bytes either side of the output stay; an empty batch and an unaligned q view work."""
    c = case
    seen = {fl: set() for fl in MASKS}
    for n in NS:
        q = c.q[:n]
        pos = ops.fk_points(c.ps, q)
        for fl in MASKS:
            for margin in margins_of(fl):
                want = ops.collision_fields(c.cm, fl, pos, margin=margin).cpu().numpy().astype(bool)
                got = ops.rollout_points_collision(c.ps, c.cm, fl, q, margin=margin)
                assert ops.last_dispatch() == "generated"
                assert got.shape == (n,) and got.dtype == torch.bool
                got = got.cpu().numpy()
                bad = np.flatnonzero(got != want)
                assert len(bad) <= max(1, n // 2000), (n, fl, margin, len(bad))
                if margin is not None:
                    ref, stable = c.oracle(fl, margin)
                    assert stable[bad].sum() == 0, (n, fl, margin, bad)
                    off = np.flatnonzero((got != ref[:n]) & stable[:n])
                    assert len(off) == 0, (n, fl, margin, off[:8])
                    if n == N_ALL:
                        seen[fl] |= set(np.unique(ref).tolist())
        # sentinels: the launch writes its n bytes and nothing else
        buf = torch.full((n + 256,), 0xAB, device=DEV, dtype=torch.uint8)
        _raw_collision(c.ps, c.cm, ALLF, q, None, buf[128:])
        assert bool((buf[:128] == 0xAB).all()) and bool((buf[128 + n:] == 0xAB).all())
        np.testing.assert_array_equal(buf[128:128 + n].cpu().numpy().astype(bool), ops.rollout_points_collision(c.ps, c.cm, ALLF, q).cpu().numpy())
    for fl in (FIELD_SELF, FIELD_OBJECTS, ALLF):                # both outcomes occurred (self: at SELF_MARGIN)
        assert seen[fl] == {False, True}, fl
    # an empty batch; (B, H, D) input; q at a 4-byte offset from its allocation
    assert ops.rollout_points_collision(c.ps, c.cm, ALLF, torch.empty((0, 7), device=DEV)).shape == (0,)
    assert ops.rollout_points_collision(c.ps, c.cm, ALLF, torch.empty((0, 64, 7), device=DEV)).shape == (0, 64)
    ref7 = ops.rollout_points_collision(c.ps, c.cm, ALLF, c.q[:1000], margin=0.07)
    np.testing.assert_array_equal(ops.rollout_points_collision(c.ps, c.cm, ALLF, c.q[:1000].reshape(8, 125, 7), margin=0.07).cpu().numpy().reshape(-1),
                                  ref7.cpu().numpy())
    raw = torch.empty(1000 * 7 + 1, device=DEV)
    view = raw[1:].view(1000, 7)
    view.copy_(c.q[:1000])
    assert view.data_ptr() % 16 == 4
    np.testing.assert_array_equal(ops.rollout_points_collision(c.ps, c.cm, ALLF, view, margin=0.07).cpu().numpy(), ref7.cpu().numpy())
    with pytest.raises(ValueError):
        ops.rollout_points_collision(c.ps, c.cm, ALLF, torch.zeros(4, 14, device=DEV))


@pytest.mark.parametrize("case", [(r, "spheres3d") for r in ROBOTS], indirect=True, ids=lambda c: c[0])
def test_moved_base(case):
    """k_pcoll_bg: the robot's base moved (fresh handles; the task's stay at the identity) -- two-step path and fp64 oracle."""
    c = case
    kin = copy.deepcopy(c.kin)
    kin.set_base_pose(MOVED_BASE)
    h = ops.ModelHandle(kin)
    h.set_base_pose(kin.base_R, kin.base_t)
    ps, cm = ops.PointSetHandle(h, c.pl, c.po, DEV), ops.CostHandle(c.spec, DEV)
    orc = c.oracle_lib.Oracle(kin, _host_spec(c.spec))
    n = 1000
    q = c.q[:n]
    pos64 = orc.fk_points(c.pl, c.po, c.q_np[:n].astype(np.float64), "f64")
    assert np.abs(pos64 - c.pos64[:n]).max() > 0.05             # the base did move
    pos = ops.fk_points(ps, q)
    for fl in (FIELD_SELF, FIELD_OBJECTS | FIELD_WS, ALLF):
        for margin in margins_of(fl):
            want = ops.collision_fields(cm, fl, pos, margin=margin).cpu().numpy().astype(bool)
            got = ops.rollout_points_collision(ps, cm, fl, q, margin=margin).cpu().numpy()
            assert ops.last_dispatch() == "generated"
            bad = np.flatnonzero(got != want)
            assert len(bad) <= max(1, n // 2000), (fl, margin, len(bad))
            if margin is not None:
                f = lambda m: orc.collision_fields(fl, pos64, m, "f64").astype(bool)
                stable = f(margin - BAND) == f(margin + BAND)
                assert (~stable).mean() <= MAX_UNSTABLE_SHARE
                assert stable[bad].sum() == 0 and not ((got != f(margin)) & stable).any(), (fl, margin)


def _trajs(c, T, H, S, seed):
    """(T, H, S) way points: joint positions uniform in the limits, the other columns noise"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (T, H, S)).astype(np.float32)
    x[..., :7] = rng.uniform(c.q_min, c.q_max, (T, H, 7)).astype(np.float32)
    return dev(x)


@pytest.mark.parametrize("case", [(r, "spheres3d") for r in ROBOTS], indirect=True, ids=lambda c: c[0])
def test_via_mode_equals_interpolation_then_the_fused_kernel(case):
    """The via points interpolated in the kernel == interpolate_traj_via_points followed by rollout_points_collision, bit for bit;
    with the limits, the same booleans and the per-trajectory flags of the three-launch form."""
    c = case
    lim = (dev(c.q_min.astype(np.float32)), dev(c.q_max.astype(np.float32)))
    for (T, H, S, n) in ((12, 16, 7, 5), (7, 2, 7, 1), (33, 64, 14, 5), (257, 5, 9, 3), (4, 3, 7, 70)):
        x = _trajs(c, T, H, S, 100 + T)
        x[::3, H // 2, 2] = float(c.q_max[2]) + 0.25              # some way points outside the limits
        via = ops.interpolate_traj_via_points(x, num_interpolation=n)
        assert via.shape == (T, (H - 1) * n, S)
        for margin in (0.0, None):
            want = ops.rollout_points_collision(c.ps, c.cm, ALLF, via[..., :7].contiguous(), margin=margin)
            got = ops.rollout_points_collision_via(c.ps, c.cm, ALLF, x, n, margin=margin)
            assert ops.last_dispatch() == "generated"
            assert got.shape == (T, (H - 1) * n) and got.dtype == torch.bool
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=str((T, H, S, n, margin)))
            got2, flags = ops.rollout_points_collision_via(c.ps, c.cm, ALLF, x, n, margin=margin, limits=lim)
            np.testing.assert_array_equal(got2.cpu().numpy(), want.cpu().numpy())
            a = ops.traj_validate(None, x, 7, lim[0], lim[1], flags=flags)
            b = ops.traj_validate(want, x, 7, lim[0], lim[1])
            assert a.counts() == b.counts()
            np.testing.assert_array_equal(a.flags.cpu().numpy(), b.flags.cpu().numpy())
            np.testing.assert_array_equal(a.idx.cpu().numpy(), b.idx.cpu().numpy())
        if T == 12:
            assert {0, 2} <= set(np.unique(b.flags.cpu().numpy() & 2).tolist())       # inside and outside both occurred


class _routing:
    """TRK_POINTS_COLLISION_FUSED for a block: "0" the task's routing before the fused kernels, "1" the fused kernels whatever the
    measured default of the model and call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = os.environ.get("TRK_POINTS_COLLISION_FUSED")
        os.environ["TRK_POINTS_COLLISION_FUSED"] = self.value

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["TRK_POINTS_COLLISION_FUSED"]
        else:
            os.environ["TRK_POINTS_COLLISION_FUSED"] = self.prev
        return False


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("case", [(r, "spheres3d") for r in ROBOTS], indirect=True, ids=lambda c: c[0])
def test_task_routing_equals_the_two_step_routing(case):
    """compute_collision and get_trajs_collision_and_free(return_indices=True) through the fused kernels == the routing under
    TRK_POINTS_COLLISION_FUSED=0: equal tensors and index lists, free, colliding and out-of-limits trajectories all present; with the
    model's generated kernels switched off the via op declines and the task's answer stays."""
    c, task = case, case.task
    with _routing("0"):
        want_cc = task.compute_collision(c.q)
        free_q = c.q[~task.compute_collision(c.q, margin=0.).reshape(-1)]
    with _routing("1"):
        got_cc = task.compute_collision(c.q)
    assert ops.last_dispatch() == "generated"
    assert torch.equal(got_cc, want_cc) and got_cc.dtype == torch.bool and bool(got_cc.any()) and not bool(got_cc.all())
    q3 = c.q[:4096].reshape(64, 64, 7)
    with _routing("0"):
        want3 = task.compute_collision(q3, margin=0.07)
    with _routing("1"):
        assert torch.equal(task.compute_collision(q3, margin=0.07), want3) and want3.shape == (64, 64)
    # the model's generated kernels off: the library itself takes the two launches through the op's scratch, same bytes
    c.model.enable_specialized(False)
    try:
        fb = ops.rollout_points_collision(c.ps, c.cm, ALLF, q3, margin=0.07)
        assert ops.last_dispatch() == "table-driven"
        pos_t = ops.fk_points(c.ps, q3.reshape(-1, 7))
        want_t = ops.collision_fields(c.cm, ALLF, pos_t, margin=0.07).reshape(64, 64)
        with _routing("1"):
            fb_task = task.compute_collision(q3, margin=0.07)
    finally:
        c.model.enable_specialized(True)
    assert torch.equal(fb, want_t) and torch.equal(fb_task, want_t) and fb.dtype == torch.bool
    assert free_q.shape[0] > 300
    gen = torch.Generator(device=DEV).manual_seed(7)
    for (T, H, n) in ((37, 64, 5), (1, 2, 1), (203, 3, 2)):
        # a third of the trajectories wander off a collision-free configuration in small steps, the others are uniform draws (they
        # collide); every fifth gets a way point beyond a joint limit
        start = free_q[torch.arange(T, device=DEV) % free_q.shape[0]]
        walk = start[:, None, :] + 0.01 * torch.randn(T, H, 7, device=DEV, generator=gen).cumsum(1)
        trajs = _trajs(c, T, H, 7, 300 + T)
        trajs[::3] = walk[::3]
        lo, hi = dev(c.q_min.astype(np.float32)), dev(c.q_max.astype(np.float32))
        trajs = torch.minimum(torch.maximum(trajs, lo + 1e-3), hi - 1e-3)
        trajs[::5, H - 1, 3] = float(c.q_max[3]) + 0.2
        with _routing("0"):
            want = task.get_trajs_collision_and_free(trajs, return_indices=True, num_interpolation=n)
        with _routing("1"):
            got = task.get_trajs_collision_and_free(trajs, return_indices=True, num_interpolation=n)
        assert ops.last_dispatch() == "generated"
        _same(got, want)
        if T == 37:
            tc, ci, tf, fi, wp = got
            assert tf is not None and tc is not None and 0 < fi.shape[0] < T and bool(wp.any()) and not bool(wp.all())
            lim = (lo, hi)
            res = ops.rollout_points_collision_via(c.ps, c.cm, ALLF, trajs, n, margin=0., limits=lim)
            flags = ops.traj_validate(None, trajs, 7, lo, hi, flags=res[1]).flags.cpu().numpy()
            assert (flags == 0).any() and (flags & 1).any() and (flags & 2).any()       # free, colliding, outside the limits
        # the model's generated kernels off: the via op declines, the task interpolates first and answers the same
        c.model.enable_specialized(False)
        try:
            assert ops.rollout_points_collision_via(c.ps, c.cm, ALLF, trajs, n, margin=0.) is None
            with _routing("1"):
                off = task.get_trajs_collision_and_free(trajs, return_indices=True, num_interpolation=n)
        finally:
            c.model.enable_specialized(True)
        _same(off, want)


def test_run_time_unit_gets_the_boolean_kernel(oracle_lib):
    """A Panda holding a box of another size (the grasp golden's point set, stretched: no ahead-of-time unit) compiled at run time
    (jit.specialize_points): its boolean kernels come with it and hold against the fp64 oracle."""
    from torch_robotics_amd import jit
    assert jit.hipcc_available()           # (the hipRTC fall-back carries no boolean kernel: jit.specialize_points)
    m, pl, po, spec = grasp_panda_setup()
    po = (po * np.float32(1.25)).astype(np.float32)
    ident = jit.specialize_points(m, pl, po, spec)
    assert ident and (jit.JIT_DIR / f"spec_{ident}_coll.so").exists()
    h = ops.ModelHandle(m)
    ps, cm = ops.PointSetHandle(h, pl, po, DEV), ops.CostHandle(spec, DEV)
    assert ps.specialized
    n = 257
    lim = gold("panda_robot")["q_limits"].astype(np.float64)
    lim = lim if lim.shape[0] == 2 else lim.T
    q_np = np.random.default_rng(11).uniform(lim[0], lim[1], (n, 7)).astype(np.float32)
    orc = oracle_lib.Oracle(m, spec)
    pos64 = orc.fk_points(pl, po, q_np.astype(np.float64), "f64")
    for fl in MASKS:
        for margin in margins_of(fl)[1:]:
            got = ops.rollout_points_collision(ps, cm, fl, dev(q_np), margin=margin).cpu().numpy()
            assert ops.last_dispatch() == "generated"
            f = lambda mm: orc.collision_fields(fl, pos64, mm, "f64").astype(bool)
            stable = f(margin - BAND) == f(margin + BAND)
            assert (~stable).mean() <= MAX_UNSTABLE_SHARE
            assert not ((got != f(margin)) & stable).any(), (fl, margin)
    x = dev(np.random.default_rng(12).uniform(lim[0], lim[1], (9, 6, 7)).astype(np.float32))
    via = ops.interpolate_traj_via_points(x, num_interpolation=3)
    np.testing.assert_array_equal(ops.rollout_points_collision_via(ps, cm, ALLF, x, 3, margin=0.).cpu().numpy(),
                                  ops.rollout_points_collision(ps, cm, ALLF, via, margin=0.).cpu().numpy())

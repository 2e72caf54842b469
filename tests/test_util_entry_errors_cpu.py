"""What the FK, Jacobian, IK, field and utility entries of the C ABI answer to a bad call: the return code and the FULL
trk_last_error() text of every case of the table below, and the early TRK_OK returns.  These entries share their host path (the launch
tail, the stateless-utility form, "generated unit or table-driven kernel", the IK unit lookup: launched, run_utility, unit_or_table,
unit_tracking in csrc/trk_capi.hip); each keeps its own argument ladder and its own place for the empty-batch return, and this file
holds what a caller sees of them -- which check speaks first, and in which words.

tests/golden/util_entry_errors.json was recorded by running this same table (CASES) against the library built from the commit BEFORE
the entries were given their shared host path ("Test pack, reduce and row-scale kernels to the bit; keep -0 in fp16"):
{case id: {"rc": code, "error": text, or null where the call returns TRK_OK}}.  Re-record with PYTHONPATH = the repository and tests/
(python tests/test_util_entry_errors_cpu.py [path]) on UNCHANGED entries only.

Model and cost model are blocks of zeros that are never dereferenced beyond their own fields: a zeroed model has 0 links, 0 DOF and
its generated kernels disabled, a zeroed cost model has no objects.  PS_OWNED / PS_WIDE are point-set blocks whose head (the
DevPointSet, the blob pointer, the owning model: _PointSetHead mirrors the first fields of TrkPointSet) names MODEL as the owner, with
213 and 214 points: the 160 KiB LDS bound of trk_fk_points lies between them.  No case may reach the device or the library's
initialisation: every case carries a fault of its own, or an empty batch (or a zero-DOF model, an object-less cost model, two null
outputs) that returns before either (test_no_answer_came_from_the_device).  A zeroed model has no link, so what trk_fk_jacobian,
trk_ik_steps and trk_ik_gn_steps check behind "link out of range" is in tests/test_gpu_fk_ik_paths_bits.py."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from torch_robotics_amd import _abi, _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "util_entry_errors.json"
NAN, INF = float("nan"), float("inf")
F32, F16 = 0, 1                                             # TRK_F32 / TRK_F16


class _PointSetHead(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("begin", C.c_void_p), ("n_points", C.c_int32), ("_pad", C.c_int32), ("d_blob", C.c_void_p),
                ("model", C.c_void_p)]


MODEL, CM, PS = (C.c_char * 8192)(), (C.c_char * 8192)(), (C.c_char * 8192)()      # stand for TrkModel* / TrkCostModel* / TrkPointSet*
BUF = (C.c_float * 4096)()                                  # host memory standing for the device buffers, never read
SEL = (C.c_int32 * 4)(0, 0, 0, 0)
DIMS, BAD_DIMS = (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(2, 0, 2)


def _owned(n_points):
    block = (C.c_char * 8192)()
    head = _PointSetHead.from_buffer(block)
    head.n_points, head.model = n_points, C.addressof(MODEL)
    return block


PS_OWNED, PS_WIDE = _owned(213), _owned(214)

# entry -> ((parameter, value of a call that is sound up to the device), ...) in the C function's order, the stream left out
ENTRIES = {
    "trk_fk_forward": (("m", MODEL), ("q", BUF), ("n", 2), ("link_sel", None), ("n_sel", 0), ("out", BUF)),
    "trk_fk_positions": (("m", MODEL), ("q", BUF), ("n", 2), ("link_sel", None), ("n_sel", 0), ("out", BUF)),
    "trk_fk_backward": (("m", MODEL), ("q", BUF), ("g", BUF), ("n", 2), ("link_sel", None), ("n_sel", 0), ("gq", BUF)),
    "trk_fk_positions_backward": (("m", MODEL), ("q", BUF), ("g", BUF), ("n", 2), ("link_sel", None), ("n_sel", 0), ("gq", BUF)),
    "trk_fk_points": (("m", MODEL), ("ps", PS_OWNED), ("q", BUF), ("n", 2), ("out", BUF)),
    "trk_fk_points_backward": (("m", MODEL), ("ps", PS_OWNED), ("q", BUF), ("g", BUF), ("n", 2), ("gq", BUF)),
    "trk_fk_jacobian": (("m", MODEL), ("q", BUF), ("qd", None), ("n", 2), ("link", 0), ("pos", BUF), ("quat", BUF), ("lin", BUF),
                        ("ang", BUF), ("vel_lin", None), ("vel_ang", None)),
    "trk_fk_analytic_jacobian": (("m", MODEL), ("q", BUF), ("n", 2), ("J", BUF)),
    "trk_ik_step": (("m", MODEL), ("link", 0), ("H_target", BUF), ("per_sample", 0), ("lower", BUF), ("upper", BUF), ("w_jl", 300.0),
                    ("se3_eps", 0.1), ("lr", 0.01), ("step", 1), ("n", 2), ("q", BUF), ("adam_m", BUF), ("adam_v", BUF), ("loss", BUF),
                    ("valid", BUF)),
    "trk_ik_steps": (("m", MODEL), ("link", 0), ("H_target", BUF), ("per_sample", 0), ("lower", BUF), ("upper", BUF), ("w_jl", 300.0),
                     ("se3_eps", 0.1), ("lr", 0.01), ("first_step", 1), ("n_steps", 2), ("n", 2), ("q", BUF), ("adam_m", BUF),
                     ("adam_v", BUF), ("loss", BUF), ("valid", BUF)),
    "trk_ik_gn_steps": (("m", MODEL), ("link", 0), ("H_target", BUF), ("per_sample", 0), ("lower", BUF), ("upper", BUF),
                        ("damping", 1e-4), ("lm_gain", 0.1), ("step_scale", 1.0), ("se3_eps", 0.1), ("n_steps", 2), ("n", 2), ("q", BUF),
                        ("err", BUF), ("valid", BUF)),
    "trk_rotmat_to_quat": (("R", BUF), ("n", 2), ("stride", 9), ("pitch", 3), ("quat", BUF)),
    "trk_rotation_from": (("kind", 0), ("x", BUF), ("n", 2), ("R", BUF)),
    "trk_rotation_from_backward": (("kind", 0), ("x", BUF), ("gR", BUF), ("n", 2), ("gx", BUF)),
    "trk_frame_compose": (("op", 0), ("Ra", BUF), ("ta", BUF), ("na", 2), ("Rb", BUF), ("tb", BUF), ("nb", 2), ("R_out", BUF),
                          ("t_out", BUF)),
    "trk_frame_compose_backward": (("op", 0), ("Ra", BUF), ("ta", BUF), ("Rb", BUF), ("tb", BUF), ("gR", BUF), ("gt", BUF), ("n", 2),
                                   ("gRa", BUF), ("gta", BUF), ("gRb", BUF), ("gtb", BUF)),
    "trk_frame_transform_points": (("R", BUF), ("t", BUF), ("n", 2), ("points", BUF), ("P", 3), ("out", BUF)),
    "trk_frame_transform_points_backward": (("gout", BUF), ("n", 2), ("points", BUF), ("P", 3), ("gR", BUF), ("gt", BUF)),
    "trk_frame_quat_euler": (("R", BUF), ("n", 2), ("stride", 9), ("pitch", 3), ("quat", BUF), ("euler", BUF)),
    "trk_frame_quat_euler_backward": (("R", BUF), ("n", 2), ("stride", 9), ("pitch", 3), ("gquat", BUF), ("geuler", BUF), ("gR", BUF)),
    "trk_cost_fields": (("cm", CM), ("fields", 7), ("link_pos", BUF), ("n", 2), ("gcost", None), ("cost", BUF), ("g", None)),
    "trk_collision_fields": (("cm", CM), ("fields", 7), ("link_pos", BUF), ("n", 2), ("margin", NAN), ("out", BUF)),
    "trk_ee_cost": (("cm", CM), ("H", BUF), ("n", 2), ("stride", 16), ("target", None), ("per_sample", 0), ("gcost", None), ("cost", BUF),
                    ("gH", None), ("g_stride", 16)),
    "trk_traj_validate": (("wp", BUF), ("x", BUF), ("n_traj", 4), ("horizon", 8), ("state_dim", 14), ("n_waypoints", 8), ("n_dofs", 7),
                          ("q_min", BUF), ("q_max", BUF), ("inner", 0), ("flags", BUF), ("idx", BUF), ("counts", BUF),
                          ("counts_host", None), ("ticket", 0), ("gathered", None)),
    "trk_interpolate_via_points": (("x", BUF), ("n_traj", 2), ("horizon", 8), ("dim", 7), ("n_interp", 2), ("alpha", BUF), ("beta", BUF),
                                   ("out", BUF)),
    "trk_jtj": (("lin", BUF), ("ang", BUF), ("residual", BUF), ("n", 2), ("dof", 7), ("use_mfma", 0), ("JtJ", BUF), ("Jtr", BUF),
                ("damping", None), ("damping_stride", 0), ("dq", None)),
    "trk_scale_rows": (("g", BUF), ("scale", BUF), ("scale_stride", 1), ("n", 2), ("dim", 7), ("io_dtype", F32), ("out", BUF)),
    "trk_interpolate_columns": (("x", BUF), ("n", 2), ("n_in", 4), ("channels", 3), ("n_out", 2), ("src", BUF), ("w", BUF), ("out", BUF)),
    "trk_interpolate_columns_backward": (("g", BUF), ("n", 2), ("n_in", 4), ("channels", 3), ("n_out", 2), ("src", BUF), ("w", BUF),
                                         ("gx", BUF)),
    "trk_gp_prior_cost_grad": (("q", BUF), ("qd", BUF), ("batch", 2), ("horizon", 8), ("dof", 7), ("io_dtype", F32), ("dt", 0.1),
                               ("sigma", 1.0), ("weight", 1.0), ("cost", BUF), ("gq", BUF), ("gqd", BUF), ("grad_dtype", F32),
                               ("grad_scale", 1.0), ("accumulate", 0)),
    "trk_finite_difference": (("x", BUF), ("batch", 2), ("horizon", 8), ("dim", 7), ("dt", 0.1), ("method", 0), ("out", BUF)),
    "trk_traj_diff_norm_sum": (("x", BUF), ("batch", 2), ("horizon", 8), ("state_dim", 14), ("c0", 0), ("dim", 7), ("out", BUF)),
    "trk_pack_sums": (("cost", BUF), ("gq", BUF), ("grad_dtype", F32), ("grad_scale", 1.0), ("block_sums", BUF), ("traj_cost", None),
                      ("batch", 2), ("horizon", 8), ("dof", 7), ("scratch", BUF), ("packed", BUF)),
    "trk_reduce_sum": (("x", BUF), ("n", 2), ("out", BUF)),
    "trk_grid_precompute": (("cm", CM), ("dims", DIMS), ("lim_min", BUF), ("lim_max", BUF), ("sdf", BUF), ("grad", BUF)),
    "trk_sdf_points": (("cm", CM), ("points", BUF), ("n", 2), ("sdf", BUF), ("grad", None)),
}
# the parameter that holds the batch, where an entry has one: 0 there is the early TRK_OK
BATCH = {e: next((p for p, _ in ps if p in ("n", "batch", "n_traj", "na")), None) for e, ps in ENTRIES.items()}
# entries that a call sound up to the device does NOT reach it with on these blocks: what stops it
STOPPED = {"trk_fk_backward": "0 DOF", "trk_fk_positions_backward": "0 DOF", "trk_fk_points_backward": "0 DOF",
           "trk_fk_analytic_jacobian": "0 DOF", "trk_fk_jacobian": "no link", "trk_ik_step": "no link", "trk_ik_steps": "no link",
           "trk_ik_gn_steps": "no link", "trk_sdf_points": "no objects"}
# entries that initialise and launch on an empty batch: the table holds no empty sound call for them
NO_EMPTY_RETURN = ("trk_reduce_sum", "trk_traj_validate", "trk_pack_sums", "trk_grid_precompute")
BIG = 0x80000000


def _returns_early(kw):
    """do these arguments hold an empty batch (or point set), or no output at all?"""
    return any(kw.get(p) == 0 for p in ("n", "batch", "n_traj", "na", "nb", "P")) or (kw.get("quat", 1) is None and kw.get("euler", 1) is None)


def _table():
    """[(case id, entry, {parameter: value} that differs from the sound call, has a fault of its own)]"""
    t = []

    def add(entry, label, _faulty=True, **kw):
        assert set(kw) <= {p for p, _ in ENTRIES[entry]}, (entry, kw)
        if not _faulty and entry not in STOPPED and not _returns_early(kw):     # a sound variant: only with the empty batch
            assert entry not in NO_EMPTY_RETURN, entry
            kw, label = {**kw, BATCH[entry]: 0}, label + " (empty batch)"
        if not _faulty and entry == "trk_frame_compose" and kw.get("na") == 0:
            kw = {"nb": 0, **kw}                                # both sizes: 0 and 2 differ
        t.append((f"{entry}: {label}", entry, kw, _faulty))

    def ok(entry, label, **kw):
        add(entry, label, False, **kw)

    # ---- each pointer argument null (a nullable one included: the answer is then that of the sound call), and the plain sound call
    for entry, params in ENTRIES.items():
        for p, v in params:
            if v is not None and not isinstance(v, (int, float)):
                nullable = (entry, p) in (("trk_frame_quat_euler", "quat"), ("trk_frame_quat_euler", "euler"),
                                          ("trk_frame_quat_euler_backward", "gquat"), ("trk_frame_quat_euler_backward", "geuler"),
                                          ("trk_jtj", "Jtr"), ("trk_jtj", "residual"), ("trk_ik_step", "loss"), ("trk_ik_step", "valid"),
                                          ("trk_ik_steps", "loss"), ("trk_ik_steps", "valid"), ("trk_ik_gn_steps", "err"),
                                          ("trk_ik_gn_steps", "valid"), ("trk_fk_forward", "q"), ("trk_fk_positions", "q"),
                                          ("trk_fk_points", "q"), ("trk_traj_validate", "wp")) and entry not in NO_EMPTY_RETURN
                if entry == "trk_jtj" and p == "residual":
                    add(entry, "null residual with Jtr", residual=None)
                    ok(entry, "null residual and Jtr", residual=None, Jtr=None)
                elif nullable:
                    ok(entry, f"null {p}", **{p: None})
                else:
                    add(entry, f"null {p}", **{p: None})
        if entry not in NO_EMPTY_RETURN:
            ok(entry, "sound")
            if BATCH[entry]:
                add(entry, "empty batch, null buffers", entry in ("trk_interpolate_via_points", "trk_interpolate_columns",
                                                                   "trk_interpolate_columns_backward", "trk_ik_step", "trk_ik_steps",
                                                                   "trk_ik_gn_steps", "trk_fk_jacobian"),
                    **{BATCH[entry]: 0}, **{p: None for p, v in params if v is BUF})
        if BATCH[entry]:
            add(entry, "negative batch", **{BATCH[entry]: -1})
    add("trk_traj_validate", "null wp, no way points", wp=None, n_waypoints=0, x=None)
    add("trk_traj_validate", "null q_min, flags given (n_waypoints < 0)", q_min=None, n_waypoints=-8, idx=None)
    add("trk_traj_validate", "null q_min, n_dofs = 0", q_min=None, n_dofs=0, idx=None)
    add("trk_traj_validate", "empty batch, null counts", n_traj=0, counts=None)
    # ---- the FK family: model, selection, point set
    for e in ("trk_fk_forward", "trk_fk_positions", "trk_fk_backward", "trk_fk_positions_backward"):
        for ns in (0, 1, 5):
            add(e, f"link_sel given, n_sel = {ns}", link_sel=SEL, n_sel=ns)
        add(e, "null m + negative batch", m=None, n=-1)
        add(e, "negative batch + n_sel = 0", n=-1, link_sel=SEL, n_sel=0)
        add(e, "null output + n_sel = 0", **{"out" if "out" in dict(ENTRIES[e]) else "gq": None}, link_sel=SEL, n_sel=0)
        add(e, "n_sel = 0 + empty batch", link_sel=SEL, n_sel=0, n=0)
    for e in ("trk_fk_points", "trk_fk_points_backward"):
        add(e, "zeroed point set: no owner", ps=PS)
        add(e, "214 points: the tile exceeds the LDS", ps=PS_WIDE)
        add(e, "214 points + empty batch", ps=PS_WIDE, n=0)
        add(e, "214 points + negative batch", ps=PS_WIDE, n=-1)
        add(e, "null m + null ps", m=None, ps=None)
        add(e, "no owner + negative batch", ps=PS, n=-1)
    for e in ("trk_fk_jacobian", "trk_ik_step", "trk_ik_steps", "trk_ik_gn_steps"):
        add(e, "link = -1", link=-1)
        add(e, "null m + link = -1", m=None, link=-1)
        add(e, "link out of range + negative batch", n=-1)
    add("trk_fk_analytic_jacobian", "null m + negative batch", m=None, n=-1)
    # ---- rotations and frames
    for e in ("trk_rotmat_to_quat", "trk_frame_quat_euler", "trk_frame_quat_euler_backward"):
        for s in (8, 9, 16):
            ok(e, f"stride = {s}", stride=s) if s >= 9 else add(e, f"stride = {s}", stride=s)
        for p in (2, 3, 4):
            ok(e, f"pitch = {p}", pitch=p) if p >= 3 else add(e, f"pitch = {p}", pitch=p)
        add(e, "stride = 8 + empty batch", stride=8, n=0)
        add(e, "pitch = 2 + null R", pitch=2, R=None)
    add("trk_frame_quat_euler", "both outputs null: nothing to do", False, quat=None, euler=None)
    add("trk_frame_quat_euler", "both outputs null + null R", quat=None, euler=None, R=None)
    for e in ("trk_rotation_from", "trk_rotation_from_backward"):
        for k in (-1, 4):
            add(e, f"kind = {k}", kind=k)
            add(e, f"kind = {k} + empty batch", kind=k, n=0)
        for k in (0, 1, 2, 3):
            ok(e, f"kind = {k}", kind=k)
    for e in ("trk_frame_compose", "trk_frame_compose_backward"):
        for op in (-1, 3):
            add(e, f"op = {op}", op=op)
            add(e, f"op = {op} + negative batch", op=op, **{BATCH[e]: -1})
        for op in (0, 1, 2):
            ok(e, f"op = {op}", op=op)
        add(e, "the inverse, null b and a null output", op=1, Rb=None, tb=None, **({"R_out": None} if e == "trk_frame_compose" else {"gRa": None}))
    fc = "trk_frame_compose"
    add(fc, "nb = -1", nb=-1)
    add(fc, "the inverse, nb = -1, null R_out", op=1, nb=-1, R_out=None)
    add(fc, "sizes 2 and 3", nb=3)
    add(fc, "sizes 2 and 3 + null Ra", nb=3, Ra=None)
    add(fc, "sizes 0 and 3: differ, ahead of the empty return", na=0, nb=3)
    add(fc, "sizes 0 and 1", False, na=0, nb=1)
    add(fc, "sizes 3 and 0", nb=0, na=3)
    add(fc, "sizes 1 and 0", False, na=1, nb=0)
    add(fc, "sizes 1 and 3, null t_out", na=1, nb=3, t_out=None)
    add(fc, "sizes 3 and 1, null tb", na=3, nb=1, tb=None)
    add(fc, "the inverse, na = 0, nb = 3", False, op=1, na=0, nb=3)
    add(fc, "na = -1 + sizes differ", na=-1, nb=3)
    add("trk_frame_compose_backward", "negative batch + null Ra", n=-1, Ra=None)
    for e in ("trk_frame_transform_points", "trk_frame_transform_points_backward"):
        add(e, "P = -1", P=-1)
        add(e, "P = -1 + empty batch", P=-1, n=0)
        add(e, "negative batch + null points", n=-1, points=None)
    add("trk_frame_transform_points", "P = 0", False, P=0)
    add("trk_frame_transform_points", "P = 0, null buffers", False, P=0, R=None, t=None, points=None, out=None)
    add("trk_frame_transform_points_backward", "P = 0, null gout and points, null gR", P=0, gout=None, points=None, gR=None)
    # ---- the fields on given positions
    for e in ("trk_cost_fields", "trk_collision_fields"):
        for f in (0, 8, -1, 15):
            add(e, f"fields = {f}", fields=f)
            add(e, f"fields = {f} + empty batch", fields=f, n=0)
        for f in range(1, 8):
            ok(e, f"fields = {f}", fields=f)
        add(e, "null cm + fields = 0", cm=None, fields=0)
    ok("trk_collision_fields", "margin 0.07", margin=0.07)
    ee = "trk_ee_cost"
    for s in (15, 16, 17, 18, 20):
        ok(ee, f"stride = {s}", stride=s) if s in (16, 20) else add(ee, f"stride = {s}", stride=s)
        if s in (16, 20):
            ok(ee, f"gH with g_stride = {s}", gH=BUF, g_stride=s)
        else:
            add(ee, f"gH with g_stride = {s}", gH=BUF, g_stride=s)
            ok(ee, f"g_stride = {s} without gH", g_stride=s)
    add(ee, "null cm + stride = 15", cm=None, stride=15)
    add(ee, "stride = 15 + empty batch", stride=15, n=0)
    add("trk_grid_precompute", "a dimension of 0", dims=BAD_DIMS)
    add("trk_grid_precompute", "a dimension of 0 + null sdf", dims=BAD_DIMS, sdf=None)
    add("trk_sdf_points", "null cm + negative batch", cm=None, n=-1)
    # ---- trajectories
    iv = "trk_interpolate_via_points"
    for name, lo in (("horizon", 2), ("dim", 1), ("n_interp", 1)):
        add(iv, f"{name} = {lo - 1}", **{name: lo - 1})
        ok(iv, f"{name} = {lo}", **{name: lo})
        add(iv, f"{name} = {lo - 1} + empty batch", **{name: lo - 1}, n_traj=0)
    add(iv, "null alpha + empty batch", alpha=None, n_traj=0)
    for e in ("trk_interpolate_columns", "trk_interpolate_columns_backward"):
        for name in ("n_in", "channels", "n_out"):
            add(e, f"{name} = 0", **{name: 0})
            ok(e, f"{name} = 1", **{name: 1})
        add(e, "null src + empty batch", src=None, n=0)
        add(e, "n_out = 0 + empty batch", n_out=0, n=0)
    fd = "trk_finite_difference"
    for meth in (-1, 3):
        add(fd, f"method = {meth}", method=meth)
        add(fd, f"method = {meth} + empty batch", method=meth, batch=0)
    for meth in (0, 1, 2):
        ok(fd, f"method = {meth}", method=meth)
    add(fd, "dt = 0", dt=0.0)
    add(fd, "dt = 0 + empty batch", dt=0.0, batch=0)
    ok(fd, "dt = -0.5", dt=-0.5)
    ok(fd, "dt = nan: not equal to 0", dt=NAN)
    add(fd, "horizon = 0", horizon=0)
    ok(fd, "horizon = 1", horizon=1)
    add(fd, "dim = 0", dim=0)
    tn = "trk_traj_diff_norm_sum"
    add(tn, "c0 + dim = state_dim + 1", c0=8)
    ok(tn, "c0 + dim = state_dim", c0=7)
    add(tn, "c0 = -1", c0=-1)
    add(tn, "dim = 0", dim=0)
    add(tn, "horizon = 0", horizon=0)
    add(tn, "batch = 2^31", batch=BIG)
    add(tn, "c0 + dim > state_dim + empty batch", c0=8, batch=0)
    tv = "trk_traj_validate"
    add(tv, "n_traj = 2^30", n_traj=0x40000000)
    add(tv, "horizon = 0", horizon=0)
    add(tv, "state_dim = 0", state_dim=0, n_dofs=0)
    add(tv, "n_dofs = -1", n_dofs=-1)
    add(tv, "n_dofs = state_dim + 1", n_dofs=15)
    add(tv, "inner = -1", inner=-1)
    add(tv, "inner = 3 does not divide n_traj = 4", inner=3)
    add(tv, "inner = 3 + null counts, empty batch", inner=3, n_traj=0, counts=None)
    add(tv, "inner = 3 + null x", inner=3, x=None)
    add(tv, "inner = 3, n_traj = 5", inner=3, n_traj=5)
    # ---- the normal equations, the row scale, the prior, the packing, the sum
    for dof in (0, 1, 8, 9, _abi.TRK_MAX_DOFS, _abi.TRK_MAX_DOFS + 1):
        for mfma in (0, 1):
            label = f"dof = {dof}, use_mfma = {mfma}"
            ok("trk_jtj", label, dof=dof, use_mfma=mfma) if 1 <= dof <= (8 if mfma else _abi.TRK_MAX_DOFS) else \
                add("trk_jtj", label, dof=dof, use_mfma=mfma)
    add("trk_jtj", "dof = 9 with the MFMA kernel + empty batch", dof=9, use_mfma=1, n=0)
    add("trk_jtj", "dof = 9 with the MFMA kernel + null JtJ", dof=9, use_mfma=1, JtJ=None)
    add("trk_jtj", "dq without the residual", residual=None, Jtr=None, dq=BUF)
    for s in (-1, 2):
        add("trk_jtj", f"damping with damping_stride = {s}", damping=BUF, damping_stride=s)
        ok("trk_jtj", f"damping_stride = {s} without damping", damping_stride=s)
    for s in (0, 1):
        ok("trk_jtj", f"damping with damping_stride = {s}", damping=BUF, damping_stride=s)
    sr = "trk_scale_rows"
    for s in (-1, 2):
        add(sr, f"scale_stride = {s}", scale_stride=s)
        add(sr, f"scale_stride = {s} + empty batch", scale_stride=s, n=0)
    ok(sr, "scale_stride = 0", scale_stride=0)
    for d in (-1, 2):
        add(sr, f"io_dtype = {d}", io_dtype=d)
    ok(sr, "fp16", io_dtype=F16)
    add(sr, "dim = 0", dim=0)
    add(sr, "dim = 0 + io_dtype = 2", dim=0, io_dtype=2)
    gp = "trk_gp_prior_cost_grad"
    add(gp, "horizon = 0", horizon=0)
    ok(gp, "horizon = 1", horizon=1)
    add(gp, "dof = 0", dof=0)
    for d in (-1, 2):
        add(gp, f"io_dtype = {d}", io_dtype=d)
        add(gp, f"grad_dtype = {d}", grad_dtype=d)
    for name in ("dt", "sigma"):
        for v in (0.0, -1.0, NAN):
            add(gp, f"{name} = {v}", **{name: v})
    add(gp, "batch = 2^31", batch=BIG)
    ok(gp, "fp16 in, fp16 gradient", io_dtype=F16, grad_dtype=F16)
    ok(gp, "fp16 in, fp32 gradient", io_dtype=F16, grad_dtype=F32)
    add(gp, "fp32 in, fp16 gradient", io_dtype=F32, grad_dtype=F16)
    add(gp, "fp32 in, fp16 gradient + empty batch", io_dtype=F32, grad_dtype=F16, batch=0)
    for v in (0.0, -1.0, INF, NAN):
        add(gp, f"grad_scale = {v}", grad_scale=v)
        add("trk_pack_sums", f"grad_scale = {v}", grad_scale=v)
    ok(gp, "grad_scale = 1024", grad_scale=1024.0)
    add(gp, "dt = 0 + grad_scale = 0: the first ladder speaks", dt=0.0, grad_scale=0.0)
    add(gp, "null q + grad_dtype = 2: the first ladder speaks", q=None, grad_dtype=2)
    add(gp, "grad_scale = inf + empty batch", grad_scale=INF, batch=0)
    pk = "trk_pack_sums"
    add(pk, "batch = 0", batch=0)
    add(pk, "batch = 2^31", batch=BIG)
    add(pk, "horizon = 0", horizon=0)
    add(pk, "dof = 0", dof=0)
    for d in (-1, 2):
        add(pk, f"grad_dtype = {d}", grad_dtype=d)
    add(pk, "batch = 0 + grad_scale = nan", batch=0, grad_scale=NAN)
    add("trk_reduce_sum", "empty batch, null out", n=0, out=None)
    add("trk_reduce_sum", "null x + null out", x=None, out=None)
    return t


CASES = _table()


def answer(trk, entry, kw):
    """what a caller sees of one call: the code, and the error text where there is one"""
    args = [kw.get(p, v) for p, v in ENTRIES[entry]]
    rc = getattr(trk, entry)(*args, None)
    return {"rc": rc, "error": None if rc == _abi.TRK_OK else trk.trk_last_error().decode("utf-8")}


def record(path=GOLDEN):
    """writes the file the test compares against: the same table, so the two cannot drift apart"""
    trk = _lib.lib()
    got = {cid: answer(trk, e, kw) for cid, e, kw, _ in CASES}
    lines = [f"{json.dumps(cid)}: {json.dumps(v, sort_keys=True)}" for cid, v in sorted(got.items())]       # one line per case
    Path(path).write_text("{\n" + ",\n".join(lines) + "\n}\n")
    return got


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_table_and_the_recorded_file_hold_the_same_cases(golden):
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(golden)
    assert {c[1] for c in CASES} == set(ENTRIES)
    codes = {v["rc"] for v in golden.values()}
    assert codes == {_abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED}         # the table reaches every kind of answer
    assert all((v["error"] is None) == (v["rc"] == _abi.TRK_OK) for v in golden.values())


def test_no_answer_came_from_the_device(golden):
    """every case ends before the library's initialisation and before any launch: no recorded answer is a device's"""
    for cid, v in golden.items():
        assert v["rc"] not in (_abi.TRK_ERR_NO_DEVICE, _abi.TRK_ERR_HIP), cid
    for cid, entry, kw, faulty in CASES:
        # a case without a fault of its own has an empty batch, or its entry is stopped by the zeroed blocks themselves
        assert faulty or entry in STOPPED or _returns_early(kw), cid
        if not faulty:
            assert golden[cid]["rc"] == _abi.TRK_OK or (STOPPED.get(entry) == "no link" and golden[cid]["rc"] == _abi.TRK_ERR_INVALID_ARG), cid


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_call_gets_the_recorded_code_and_text(trk, golden, entry):
    got = {cid: answer(trk, e, kw) for cid, e, kw, _ in CASES if e == entry}
    assert len(got) >= 5
    wrong = {cid: (g, golden[cid]) for cid, g in got.items() if g != golden[cid]}
    assert not wrong, wrong


def test_the_early_returns_are_the_recorded_ones(golden):
    """the kept differences that a zeroed block can show: which entries answer TRK_OK to what"""
    for cid in ("trk_fk_backward: sound", "trk_fk_positions_backward: sound", "trk_fk_points_backward: sound",
                "trk_fk_analytic_jacobian: sound", "trk_sdf_points: sound", "trk_frame_quat_euler: both outputs null: nothing to do",
                "trk_frame_compose: sizes 0 and 1", "trk_frame_compose: sizes 1 and 0", "trk_frame_transform_points: P = 0"):
        assert golden[cid] == {"rc": _abi.TRK_OK, "error": None}, cid
    # trk_fk_points*: the LDS refusal speaks ahead of the empty batch
    for e in ("trk_fk_points", "trk_fk_points_backward"):
        assert golden[f"{e}: 214 points + empty batch"]["rc"] == _abi.TRK_ERR_UNSUPPORTED
        assert golden[f"{e}: sound (empty batch)" if e == "trk_fk_points" else f"{e}: sound"]["rc"] == _abi.TRK_OK
    assert golden["trk_frame_compose: sizes 0 and 3: differ, ahead of the empty return"]["error"].endswith("neither is 1")


if __name__ == "__main__":
    record(*sys.argv[1:2])

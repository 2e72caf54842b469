"""The three Jacobian entries on every bundled robot, every link and every width, against the fp64 oracle and exact integers.

trk_fk_jacobian (generated k_jac_bi / _bg in its direct and record forms, table-driven k_fk_jacobian), trk_fk_analytic_jacobian
(generated k_ajac, table-driven k_fk_analytic_jacobian) and trk_jtj (k_jtj<false>, <false, 6>, <false, 7>, <true>).  Every expected
value comes from oracle_impl.inc in fp64 or from int64 arithmetic (tests/jacobian_helpers.py; its rules are pinned on the CPU by
tests/test_jacobian_refs_cpu.py): no kernel is compared with itself or with another route alone.

Quaternion-candidate ties: tests/test_jacobian_refs_cpu.py records how many (sample, link) blocks of these inputs are tied per robot
(hab_stretch 1876 of 5896, Allegro hand 134, Tiago 62, UR10 2, UR10 + Allegro 1, the others none) and that the fp32 oracle switched
candidate only at fp64 gaps up to 1.3e-7, inside TIE_MARGIN = 8e-6.  A tied block must be the fp64 result through a member of its tie
set; every other block the oracle's own.  Nothing is excluded.

The solve: (JtJ + lambda I) dq = Jtr is held to the residual bound CHOL_BOUND (3 D + 1) 2^-24 of Higham's scale, CHOL_BOUND = 1.92 =
4 x the 0.476 the fp32 restatement of the kernel's own factorisation reaches over these cases.  lambda = 0 on a singular JtJ (any
D > 6: six rows) has no defined answer and is left out."""
import os

import numpy as np
import pytest
import torch

import jacobian_helpers as jh
from helpers import ROBOTS, model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOVED_GEO = ("dual_panda", "ur10_allegro", "hab_stretch")
MOVED_AJAC = ("dual_panda", "hab_stretch")


@pytest.fixture(scope="module")
def ops():
    from torch_robotics_amd import ops as _ops
    return _ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.cpu().numpy()


def unit_plan(robot):
    """codegen's plan of the robot's ahead-of-time unit: which kernel families it carries and in which form"""
    from torch_robotics_amd import codegen
    ident = next(k for k, (urdf, _) in codegen.SPEC_ROBOTS.items() if urdf == robot + ".urdf")
    kin, tmpl = codegen.template_for(ident)
    return codegen._LinkUnit(kin, tmpl, ident, codegen.SNAP)


_cases = {}


def case(oracle_lib, robot, moved=False):
    """Per (robot, base), computed once and never written to: the model, its oracle, q (jacobian_inputs) and a random qd, and the fp64
    references: the geometric Jacobian of every link, the FK and the analytic Jacobian."""
    key = (robot, moved)
    if key not in _cases:
        m = model(robot)
        if moved:
            m.set_base_pose(jh.MOVED_BASE)
        o = oracle_lib.Oracle(m)
        q = jh.jacobian_inputs(m)
        qd = np.random.default_rng(6).standard_normal(q.shape).astype(np.float32)
        q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
        geo = [o.jacobian(q64, qd64, link, "f64") for link in range(m.n_links)]
        _cases[key] = dict(m=m, o=o, q=q, qd=qd, geo=geo, H=o.fk(q64, "f64"), J64=o.analytic_jacobian(q64, "f64"),
                           rows=jh.batch_rows(len(q)))
    return _cases[key]


def geo_check(got, ref, rows, what):
    """One trk_fk_jacobian result against the oracle's (pos, quat, lin, ang[, vel_lin, vel_ang]) on `rows`: the project's bounds
    5e-6 max(1, |ref|max) (3e-6 for the unit axes), the quaternion through the frame rule, and columns the oracle leaves at zero
    exactly zero."""
    pos, quat, lin, ang = (host(t) for t in got[:4])
    rpos, rquat, rlin, rang, rvl, rva = (a[rows] for a in ref)
    for name, a, b, tol in (("pos", pos, rpos, 5e-6), ("lin", lin, rlin, 5e-6), ("ang", ang, rang, 3e-6)):
        assert a.shape == b.shape, (what, name)
        err = np.abs(a - b).max()
        assert err <= tol * max(1.0, float(np.abs(b).max())), (what, name, float(err))
    bad = jh.quat_accept(quat, jh.rot_from_quat64(rquat), tol=5e-6, rule="frame")
    assert len(bad) == 0, (what, "quat", bad[:8], quat[bad[:2]], rquat[bad[:2]])
    zero = (rang == 0).all(axis=(0, 1)) & (rlin == 0).all(axis=(0, 1))
    assert (lin[:, :, zero] == 0).all() and (ang[:, :, zero] == 0).all(), (what, "columns the oracle leaves at zero")
    if len(got) > 4:
        for name, a, b in (("vel_lin", host(got[4]), rvl), ("vel_ang", host(got[5]), rva)):
            err = np.abs(a - b).max()
            assert err <= 5e-6 * max(1.0, float(np.abs(b).max())), (what, name, float(err))


@pytest.mark.parametrize("robot", ROBOTS)
def test_geometric_jacobian_every_link(ops, oracle_lib, robot):
    """Every link 0 .. L-1 at every batch size through the generated kernel (qd=None), the table-driven kernel (kernels off) and
    the velocity route (want_vel=True, table-driven by construction), each against Oracle.jacobian in fp64.  q is uniform(-3, 3),
    beyond most limits, with rows exactly on a lower and an upper limit."""
    c = case(oracle_lib, robot)
    m, u = c["m"], unit_plan(robot)
    h = ops.ModelHandle(m)
    # the form the generated route runs comes from the unit plan: direct tiles up to JAC_DIRECT_MAX_DOFS, LDS records beyond
    from torch_robotics_amd import codegen
    assert h.specialized and u.jac_ok and (u.L, u.D) == (m.n_links, m.n_dofs)
    assert u.jac_direct == (m.n_dofs <= codegen.JAC_DIRECT_MAX_DOFS)
    for n, rows in c["rows"].items():
        q, qd = dev(c["q"][rows]), dev(c["qd"][rows])
        for link in range(m.n_links):
            h.enable_specialized(True)
            assert h.specialized
            geo_check(ops.fk_jacobian(h, q, None, link), c["geo"][link], rows, (robot, "generated", "direct" if u.jac_direct else "record", n, link))
            geo_check(ops.fk_jacobian(h, q, qd, link, want_vel=True), c["geo"][link], rows, (robot, "velocities", n, link))
            h.enable_specialized(False)
            assert not h.specialized
            geo_check(ops.fk_jacobian(h, q, None, link), c["geo"][link], rows, (robot, "table-driven", n, link))
    h.enable_specialized(True)
    # the plan writes every element, the zero columns included: outputs poisoned before the launch
    rows = c["rows"][130]
    for link in (0, m.n_links // 2, m.n_links - 1):
        plan = ops.JacobianPlan(h, dev(c["q"][rows]), link)
        for t in (plan.pos, plan.quat, plan.lin_jac, plan.ang_jac):
            t.fill_(7.0)
        plan.launch()
        torch.cuda.synchronize()
        geo_check((plan.pos, plan.quat, plan.lin_jac, plan.ang_jac), c["geo"][link], rows, (robot, "plan", link))


def test_record_form_robots_are_the_large_ones():
    """the four robots beyond JAC_DIRECT_MAX_DOFS (UR10 + Allegro 22, iiwa7 + Allegro 23, shadow hand 24, Tiago 18) take the record
    form, the other seven the direct one -- read off the unit plans, so a moved threshold moves the test with it"""
    forms = {robot: unit_plan(robot).jac_direct for robot in ROBOTS}
    assert sorted(r for r, direct in forms.items() if not direct) == sorted(r for r in ROBOTS if model(r).n_dofs > 16)
    assert sum(forms.values()) == 7


@pytest.mark.parametrize("robot", MOVED_GEO)
def test_geometric_jacobian_moved_base(ops, oracle_lib, robot):
    """the _bg instantiation (a base pose that is not the identity) and the table-driven kernel, every link, 65 rows"""
    c = case(oracle_lib, robot, moved=True)
    m = c["m"]
    h = ops.ModelHandle(m)
    assert h.specialized
    rows = c["rows"][65]
    q = dev(c["q"][rows])
    for on in (True, False):
        h.enable_specialized(on)
        for link in range(m.n_links):
            geo_check(ops.fk_jacobian(h, q, None, link), c["geo"][link], rows, (robot, "moved base", on, link))


def ajac_check(J, c, rows, what):
    """zero offenders of ajac_accept; columns of clamped joints and of joints off the link's path exactly zero"""
    m = c["m"]
    J = host(J)
    assert J.shape == (len(rows), m.n_links, 7, m.n_dofs), what
    assert np.isfinite(J).all(), what
    res = jh.ajac_accept(J, c["q"][rows], c["o"], J64=c["J64"][rows], H64=c["H"][rows])
    assert len(res["pos"]) == 0, (what, "position rows", res["pos"][:8])
    assert len(res["quat"]) == 0, (what, "quaternion rows", res["quat"][:8], int(res["tied"].sum()))
    clamped = ~jh.pass_mask(m, c["q"][rows])                       # (n, D)
    assert (J.transpose(0, 3, 1, 2)[clamped] == 0).all(), (what, "clamped columns")
    assert (J.transpose(0, 1, 3, 2)[:, ~jh.chain_mask(m)] == 0).all(), (what, "off-path columns")
    return res


@pytest.mark.parametrize("robot", ROBOTS)
def test_analytic_jacobian_every_robot(ops, oracle_lib, robot):
    """trk_fk_analytic_jacobian with the kernels on (generated k_ajac where the unit has one) and off, every batch size, through
    ajac_accept with no offender; and once through the C entry on a NaN-filled J."""
    from torch_robotics_amd._lib import check, lib
    c = case(oracle_lib, robot)
    m, u = c["m"], unit_plan(robot)
    h = ops.ModelHandle(m)
    assert h.specialized
    assert u.ajac_ok == (m.n_dofs <= 16 and m.n_links <= 24)
    tied = 0
    for on in (True, False):
        h.enable_specialized(on)
        for n, rows in c["rows"].items():
            res = ajac_check(ops.fk_analytic_jacobian(h, dev(c["q"][rows])), c, rows, (robot, "generated" if on and u.ajac_ok else "table-driven", n))
            tied = max(tied, int(res["tied"].sum()))
        rows = c["rows"][65]
        q = dev(c["q"][rows])
        J = torch.full((65, m.n_links, 7, m.n_dofs), float("nan"), device=DEV)
        check(lib().trk_fk_analytic_jacobian(h._h, q.data_ptr(), 65, J.data_ptr(), torch.cuda.current_stream().cuda_stream), "trk_fk_analytic_jacobian")
        torch.cuda.synchronize()
        assert not torch.isnan(J).any(), (robot, on)                # link 0's block and every off-path zero are written
        ajac_check(J, c, rows, (robot, on, "NaN-filled"))
    h.enable_specialized(True)
    print(f"{robot}: {tied} tied blocks in the 130-row batch")


@pytest.mark.parametrize("robot", MOVED_AJAC)
def test_analytic_jacobian_moved_base(ops, oracle_lib, robot):
    c = case(oracle_lib, robot, moved=True)
    h = ops.ModelHandle(c["m"])
    for on in (True, False):
        h.enable_specialized(on)
        for n in (65, 130):
            rows = c["rows"][n]
            ajac_check(ops.fk_analytic_jacobian(h, dev(c["q"][rows])), c, rows, (robot, "moved base", on, n))


def test_analytic_jacobian_panda_near_tie(ops, oracle_lib):
    """q1 = +-pi/2 + d: link 1's candidates 0 and 3 tie (opposite quaternions at -pi/2).  Rows with |d| <= 3e-6 lie inside the margin and
    may take either; rows at |d| = 1e-5 (gap 1.4e-5) lie outside and must take the oracle's."""
    m = model("panda_arm_no_gripper")
    o = oracle_lib.Oracle(m)
    q, ds = jh.panda_near_tie_q()
    q64 = q.astype(np.float64)
    c = dict(m=m, o=o, q=q, H=o.fk(q64, "f64"), J64=o.analytic_jacobian(q64, "f64"))
    ts = jh.tie_set(c["H"][:, 1, :3, :3])
    out = np.abs(ds) > 3e-6
    assert (ts[~out].sum(-1) == 2).all() and (ts[out].sum(-1) == 1).all()
    h = ops.ModelHandle(m)
    rows = np.arange(len(q))
    for on in (True, False):
        h.enable_specialized(on)
        J = ops.fk_analytic_jacobian(h, dev(q))
        ajac_check(J, c, rows, ("near tie", on))
        assert np.abs(host(J)[out, 1, 3:] - c["J64"][out, 1, 3:]).max() <= 5e-6, on


# ---------------------------------------------------------------------------------------------------------------------------
# trk_jtj
# ---------------------------------------------------------------------------------------------------------------------------
class generic_kernel:
    """TRK_EXP_JTJ_GENERIC=1 around a call: D = 6 and 7 take the runtime-D kernel; the variable is restored on the way out"""

    def __enter__(self):
        self.prev = os.environ.get("TRK_EXP_JTJ_GENERIC")
        os.environ["TRK_EXP_JTJ_GENERIC"] = "1"

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["TRK_EXP_JTJ_GENERIC"]
        else:
            os.environ["TRK_EXP_JTJ_GENERIC"] = self.prev
        return False


def jtj_routes(ops, D):
    """(name, call) of every kernel that serves width D: call(*args, **kw) = ops.jtj(..., mfma=...) under the route's settings"""
    def plain(*a, **k):
        return ops.jtj(*a, mfma=False, **k)

    def mfma(*a, **k):
        return ops.jtj(*a, mfma=True, **k)

    def generic(*a, **k):
        with generic_kernel():
            return ops.jtj(*a, mfma=False, **k)

    return [("per-lane", plain)] + ([("mfma", mfma)] if D <= 8 else []) + ([("runtime-D", generic)] if D in (6, 7) else [])


def offset_view(a, pad=1):
    """the array's values as a device view `pad` floats into a larger buffer: a pointer that is not 16-byte aligned"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + pad + 3, device=DEV, dtype=torch.float32)
    v = buf[pad:pad + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * pad
    return v


@pytest.mark.parametrize("D", jh.JTJ_WIDTHS)
def test_jtj_integer_cases_bit_equal(ops, D):
    """Integer-valued Jacobians and residuals: JtJ and Jtr have one right answer in fp32 whatever the order of the sums, and every
    kernel must give it to the bit, with aligned pointers and with lin / ang / JtJ one float into a buffer (the scalar load and store
    branches of full tiles)."""
    from torch_robotics_amd._lib import check, lib
    for n in jh.BATCHES:
        lin, ang, r, JtJ_i, Jtr_i = jh.jtj_int_case(n, D, seed=100 + D)
        for name, call in jtj_routes(ops, D):
            for how, (l, a) in (("aligned", (dev(lin), dev(ang))), ("offset", (offset_view(lin), offset_view(ang)))):
                JtJ, Jtr = call(l, a, dev(r))
                assert len(jh.int_mismatch(host(JtJ), JtJ_i)) == 0, (name, how, n, jh.int_mismatch(host(JtJ), JtJ_i)[:6])
                assert len(jh.int_mismatch(host(Jtr), Jtr_i)) == 0, (name, how, n, jh.int_mismatch(host(Jtr), Jtr_i)[:6])
                assert len(jh.int_mismatch(host(call(l, a)), JtJ_i)) == 0, (name, how, n, "no residual")
        # the C entry with JtJ itself one float into a poisoned buffer
        for mfma in ((0, 1) if D <= 8 else (0,)):
            l, a, rr = offset_view(lin), offset_view(ang), dev(r)
            out = torch.full((n * D * D + 8,), float("nan"), device=DEV)
            jtr = torch.full((n * D + 8,), float("nan"), device=DEV)
            check(lib().trk_jtj(l.data_ptr(), a.data_ptr(), rr.data_ptr(), n, D, mfma, out.data_ptr() + 4, jtr.data_ptr() + 4, None, 0, None,
                                torch.cuda.current_stream().cuda_stream), "trk_jtj")
            torch.cuda.synchronize()
            o, j = host(out), host(jtr)
            assert len(jh.int_mismatch(o[1:1 + n * D * D].reshape(n, D, D), JtJ_i)) == 0, (mfma, n)
            assert len(jh.int_mismatch(j[1:1 + n * D].reshape(n, D), Jtr_i)) == 0, (mfma, n)
            assert np.isnan(o[0]) and np.isnan(o[1 + n * D * D:]).all() and np.isnan(j[0]) and np.isnan(j[1 + n * D:]).all(), (mfma, n)


@pytest.mark.parametrize("D", jh.JTJ_WIDTHS)
def test_jtj_float_and_solve_cases(ops, D):
    """Random-normal Jacobians: JtJ and Jtr within the project's 2e-6 max(1, |ref|max) of fp64 numpy and JtJ exactly symmetric; the
    damped step within the residual bound of tests/test_jacobian_refs_cpu.py for lambda = 1e-2, 1 and one lambda per sample."""
    for n in jh.BATCHES:
        lin, ang, r, J, JtJ64, Jtr64 = jh.jtj_float_case(n, D, seed=200 + D)
        for name, call in jtj_routes(ops, D):
            JtJ, Jtr = call(dev(lin), dev(ang), dev(r))
            assert JtJ.shape == (n, D, D) and Jtr.shape == (n, D)
            assert np.abs(host(JtJ) - JtJ64).max() <= 2e-6 * max(1.0, np.abs(JtJ64).max()), (name, n)
            assert np.abs(host(Jtr) - Jtr64).max() <= 2e-6 * max(1.0, np.abs(Jtr64).max()), (name, n)
            assert torch.equal(JtJ, JtJ.transpose(1, 2)), (name, n)
            for lam in jh.solve_lambdas(n, seed=300 + D):
                J2, r2, dq = call(dev(lin), dev(ang), dev(r), damping=dev(lam), solve=True)
                assert torch.equal(J2, JtJ) and torch.equal(r2, Jtr), (name, n)
                dq = host(dq)
                assert np.isfinite(dq).all(), (name, n)
                res, scale = jh.chol_residual(JtJ64, Jtr64, lam, dq, J, r)
                ratio = float((res / ((3 * D + 1) * 2.0 ** -24 * scale)).max())
                assert ratio <= jh.CHOL_BOUND, (name, n, len(lam), ratio)


@pytest.mark.parametrize("D", (1, 6, 7, 8, 13, 22))
def test_jtj_zero_jacobian(ops, D):
    """J = 0 with lambda > 0: JtJ = 0, Jtr = 0, dq = 0, no NaN"""
    n = 65
    z = torch.zeros((n, 3, D), device=DEV)
    r = dev(np.random.default_rng(9).standard_normal((n, 6)).astype(np.float32))
    for name, call in jtj_routes(ops, D):
        for lam in (np.float32([1e-2]), np.linspace(1e-2, 1.0, n).astype(np.float32)):
            JtJ, Jtr, dq = call(z, z, r, damping=dev(lam), solve=True)
            assert (JtJ == 0).all() and (Jtr == 0).all() and (dq == 0).all(), name


def test_jtj_refusals(ops):
    """D = 23 and 32 are inside TRK_MAX_DOFS, but their two tiles pass the 160 KiB of LDS: refused, and nothing is launched (the
    poisoned outputs stay as they were); D = 22 is the widest that runs; the MFMA kernel refuses D = 9."""
    from torch_robotics_amd import _abi
    from torch_robotics_amd._lib import lib
    n = 65
    for D in (23, 32):
        lin, ang, r = (dev(a) for a in jh.jtj_float_case(n, D, seed=1)[:3])
        with pytest.raises(NotImplementedError, match="tiles exceed"):
            ops.jtj(lin, ang, r)
        out = torch.full((n, D, D), float("nan"), device=DEV)
        jtr = torch.full((n, D), float("nan"), device=DEV)
        rc = lib().trk_jtj(lin.data_ptr(), ang.data_ptr(), r.data_ptr(), n, D, 0, out.data_ptr(), jtr.data_ptr(), None, 0, None,
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == _abi.TRK_ERR_UNSUPPORTED
        assert torch.isnan(out).all() and torch.isnan(jtr).all()
    lin, ang, r = (dev(a) for a in jh.jtj_float_case(n, 9, seed=1)[:3])
    with pytest.raises(NotImplementedError):
        ops.jtj(lin, ang, r, mfma=True)


def test_jtj_robot_case(ops, oracle_lib):
    """UR10 + Allegro's ee_link Jacobian (D = 22, config 4's step: the two tiles take exactly 160 KiB) through fk_jacobian, jtj and the
    solve, against fp64 numpy on the ORACLE's Jacobian.  The kernel's input is the fp32 Jacobian, within e = 5e-6 max(1, |J|max) of
    the oracle's per entry (test_geometric_jacobian_every_link), so an entry of JtJ carries 6 (2 |J|max e + e^2) of input error on
    top of the kernel's own 2e-6 max(1, |ref|max), an entry of Jtr 6 e |r|max, and the residual of the oracle's system as much times
    D |dq|max."""
    c = case(oracle_lib, "ur10_allegro")
    m = c["m"]
    link = m.name_to_idx["ee_link"]
    h = ops.ModelHandle(m)
    rows = c["rows"][130]
    _, _, lin64, ang64, _, _ = (a[rows] for a in c["geo"][link])
    J = np.concatenate([lin64, ang64], 1)
    D, n = m.n_dofs, len(rows)
    assert D == 22
    r = np.random.default_rng(10).standard_normal((n, 6)).astype(np.float32)
    JtJ64, Jtr64 = np.einsum("nki,nkj->nij", J, J), np.einsum("nki,nk->ni", J, r.astype(np.float64))
    jmax, rmax = float(np.abs(J).max()), float(np.abs(r).max())
    e = 5e-6 * max(1.0, jmax)
    eA, eb = 6 * (2 * jmax * e + e * e), 6 * e * rmax
    _, _, lin, ang = ops.fk_jacobian(h, dev(c["q"][rows]), None, link)
    for lam in jh.solve_lambdas(n, seed=11):
        JtJ, Jtr, dq = ops.jtj(lin, ang, dev(r), damping=dev(lam), solve=True)
        assert np.abs(host(JtJ) - JtJ64).max() <= 2e-6 * max(1.0, np.abs(JtJ64).max()) + eA
        assert np.abs(host(Jtr) - Jtr64).max() <= 2e-6 * max(1.0, np.abs(Jtr64).max()) + eb
        dq = host(dq)
        res, scale = jh.chol_residual(JtJ64, Jtr64, lam, dq, J, r)
        assert (res <= jh.chol_bound(D) * scale + D * eA * np.abs(dq).max(-1) + eb).all()

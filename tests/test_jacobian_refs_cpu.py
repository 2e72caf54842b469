"""The references and acceptance rules of tests/test_gpu_jacobians.py (tests/jacobian_helpers.py), pinned on the CPU: they reproduce the
oracle, the oracle's own fp32 arithmetic stays inside them, and each of them rejects the planted fault it exists to catch."""
import numpy as np
import pytest

import jacobian_helpers as jh
from helpers import ROBOTS, model

# What the oracle gives on the GPU tests' own inputs (jacobian_inputs: 130 rows uniform(-3, 3), seed 5, and 4 limit rows), per robot:
# (sample, link) blocks whose tie set has more than one member, links tied in every sample, blocks where the fp32 oracle's analytic
# Jacobian differs from the fp64 oracle's by more than 1e-4 (all of them tied blocks).  The largest fp64 gap between the two leading
# q_abs at which the fp32 oracle switched candidate: 1.27e-7 (Tiago; hab_stretch 6.2e-8), 60 times inside TIE_MARGIN = 8e-6; the
# smallest gap of an untied block is 1.41e-5 (UR10).
TIE_CENSUS = {                                             # robot: (tied blocks, links tied throughout, fp32 / fp64 disagreements)
    "allegro_hand": (134, 1, 0), "dual_panda": (0, 0, 0), "hab_stretch": (1876, 14, 142), "iiwa7": (0, 0, 0), "iiwa7_allegro": (0, 0, 0),
    "panda_arm_hand": (0, 0, 0), "panda_arm_no_gripper": (0, 0, 0), "shadow_hand": (0, 0, 0),
    "tiago_dual_holobase_minimal_holonomic": (62, 0, 5), "ur10": (2, 0, 0), "ur10_allegro": (1, 0, 0)}
LARGEST_SWITCH_GAP = 1.3e-7


@pytest.fixture(scope="module")
def cases(oracle_lib):
    """per robot, computed once: the model, its oracle, the GPU tests' q, the fp64 FK and the two oracles' analytic Jacobians"""
    out = {}
    for robot in ROBOTS:
        m = model(robot)
        o = oracle_lib.Oracle(m)
        q = jh.jacobian_inputs(m)
        q64 = q.astype(np.float64)
        out[robot] = dict(m=m, o=o, q=q, H=o.fk(q64, "f64"), J64=o.analytic_jacobian(q64, "f64"), J32=o.analytic_jacobian(q, "f32"))
    return out


@pytest.mark.parametrize("robot", ROBOTS)
def test_helpers_reproduce_the_oracle(cases, oracle_lib, robot):
    """quat_jvp_through with the oracle's candidate is Oracle.analytic_jacobian's quaternion rows; quat_candidates' arg-max row is
    Oracle.rotmat_to_quat; a tie set with no margin is that arg-max alone."""
    c = cases[robot]
    R = c["H"][..., :3, :3]
    qa, cand = jh.quat_candidates(R)
    best = qa.argmax(-1)
    jvp = jh.quat_jvp_through(R[:, :, None], jh.rotation_perturbations(c["m"], c["q"], c["H"]), best[:, :, None])
    assert np.abs(jvp.transpose(0, 1, 3, 2) - c["J64"][:, :, 3:]).max() < 1e-12
    quat = oracle_lib.Oracle.rotmat_to_quat(R.reshape(-1, 9), "f64").reshape(R.shape[:2] + (4,))
    mine = np.take_along_axis(cand, best[..., None, None] + np.zeros((1, 4), np.int64), -2)[..., 0, :]
    assert np.abs(mine - quat).max() < 1e-12
    assert len(jh.quat_accept(quat.reshape(-1, 4), R.reshape(-1, 3, 3), margin=0.0, tol=1e-12)) == 0
    # Frame.get_quaternion, the geometric Jacobian's: its branch is a candidate of the same four
    for link in (0, c["m"].n_links // 2, c["m"].n_links - 1):
        _, quat_f, *_ = c["o"].jacobian(c["q"].astype(np.float64), None, link, "f64")
        Rf = jh.rot_from_quat64(quat_f)
        # (R_fixed is stored in fp32: the oracle's fp64 rotations are orthonormal to 1e-8 only, and so is Rf's agreement with them)
        assert len(jh.quat_accept(quat_f, Rf, margin=0.0, tol=1e-7, rule="frame")) == 0
        k = jh.frame_choice(Rf)
        assert np.array_equal(jh.frame_tie_set(Rf, 0.0), np.arange(4) == k[:, None])


@pytest.mark.parametrize("robot", ROBOTS)
def test_tie_census_and_the_fp32_oracle_inside_the_rule(cases, robot):
    """The condition under which the rule can be asked of a kernel at all: the reference's own fp32 arithmetic passes it with no
    offender, and everywhere it disagrees with fp64 (> 1e-4) lies inside the margin.  Measured (TIE_CENSUS above): hab_stretch 1876 tied
    blocks of 5896 (14 links tied for every q) with 142 disagreements, Allegro hand 134 (one link) with none, Tiago 62 with 5, UR10 2,
    UR10 + Allegro 1, the other six robots none.  The largest fp64 gap between the two leading q_abs at which the fp32 oracle
    switched candidate is 1.27e-7 (Tiago; hab_stretch 6.2e-8) against TIE_MARGIN = 8e-6; the smallest gap of any untied block is
    1.41e-5 (UR10)."""
    c = cases[robot]
    R = c["H"][..., :3, :3]
    tied = jh.tie_set(R).sum(-1) > 1
    dis = np.abs(c["J32"].astype(np.float64) - c["J64"]).max(axis=(2, 3)) > 1e-4
    qa = np.sort(jh.quat_candidates(R)[0], -1)
    gap = qa[..., -1] - qa[..., -2]
    print(f"{robot}: {int(tied.sum())} tied blocks of {tied.size}, {int(tied.all(0).sum())} links tied throughout, {int(dis.sum())} fp32 / fp64 "
          f"disagreements, largest switching gap {gap[dis].max() if dis.any() else 0.0:.3g}, smallest untied gap {gap[~tied].min():.3g}")
    assert (int(tied.sum()), int(tied.all(0).sum()), int(dis.sum())) == TIE_CENSUS[robot]
    assert not (dis & ~tied).any()
    if dis.any():
        assert gap[dis].max() <= LARGEST_SWITCH_GAP
    assert gap[~tied].min() > jh.TIE_MARGIN
    res = jh.ajac_accept(c["J32"], c["q"], c["o"], J64=c["J64"])
    assert len(res["pos"]) == 0 and len(res["quat"]) == 0
    assert np.array_equal(res["tied"], tied)
    # the fp32 oracle's geometric quaternion inside the frame rule, on three links
    for link in (0, c["m"].n_links // 2, c["m"].n_links - 1):
        quat64 = c["o"].jacobian(c["q"].astype(np.float64), None, link, "f64")[1]
        quat32 = c["o"].jacobian(c["q"], None, link, "f32")[1]
        assert len(jh.quat_accept(quat32, jh.rot_from_quat64(quat64), rule="frame")) == 0


def _untied_block(c, link_from=1):
    """(sample, link) of a block whose tie set has one member and whose link has a revolute joint above it that passes"""
    tied = jh.tie_set(c["H"][..., :3, :3]).sum(-1) > 1
    live = np.abs(c["J64"][:, :, 3:]).max(axis=(2, 3)) > 1e-2
    s, i = np.argwhere(~tied & live & (np.arange(tied.shape[1]) >= link_from)[None, :])[0]
    return int(s), int(i)


@pytest.mark.parametrize("robot", ["panda_arm_no_gripper", "dual_panda", "hab_stretch", "ur10_allegro"])
def test_ajac_accept_rejects_planted_faults(cases, robot):
    """Each fault in an otherwise exact array (the fp64 oracle's own, which passes) is found, at its block."""
    c = cases[robot]
    J, q, o = c["J64"], c["q"], c["o"]

    def offenders(Jbad):
        r = jh.ajac_accept(Jbad, q, o, J64=J)
        return {tuple(v) for v in r["pos"]}, {tuple(v) for v in r["quat"]}

    assert offenders(J) == (set(), set())
    s, i = _untied_block(c)
    d = int(np.argmax(np.abs(J[s, i, 3:]).max(0)))                      # a column of that block with a live quaternion part
    # one position element off by 1e-4
    B = J.copy(); B[s, i, 1, d] += 1e-4
    assert offenders(B) == ({(s, i)}, set())
    # a quaternion block negated on an untied link
    B = J.copy(); B[s, i, 3:] *= -1
    assert offenders(B) == (set(), {(s, i)})
    # one column zeroed
    B = J.copy(); B[s, i, :, d] = 0
    pb, qb = offenders(B)
    assert (s, i) in qb and pb <= {(s, i)} and qb == {(s, i)}
    # two columns swapped: d and another column of the block that differs from it
    d2 = int(np.argmax(np.abs(J[s, i] - J[s, i, :, d:d + 1]).max(0)))
    B = J.copy(); B[s, i][:, [d, d2]] = B[s, i][:, [d2, d]]
    pb, qb = offenders(B)
    assert (s, i) in (pb | qb) and (pb | qb) == {(s, i)}
    # one link's block written to the next link
    if i + 1 < J.shape[1]:
        B = J.copy(); B[s, i + 1] = J[s, i]; B[s, i] = 0
        pb, qb = offenders(B)
        assert (s, i) in (pb | qb) and (pb | qb) <= {(s, i), (s, i + 1)}
    # loosened by hand once: with quat_tol=3.0 the negated block passes, with pos_tol=1e-3 the displaced position does
    B = J.copy(); B[s, i, 3:] *= -1
    assert len(jh.ajac_accept(B, q, o, J64=J, quat_tol=3.0)["quat"]) == 0


def test_tied_block_accepts_either_member_and_nothing_else(cases):
    """hab_stretch's structural ties, at a block where the fp32 and the fp64 oracle part ways: the rows through either member of the
    tie set are accepted and differ by more than 1e-3 (opposite quaternions); anything between them is refused, and with no margin
    only the oracle's own member passes."""
    c = cases["hab_stretch"]
    R = c["H"][..., :3, :3]
    ts = jh.tie_set(R)
    dR = jh.rotation_perturbations(c["m"], c["q"], c["H"])
    dis = np.abs(c["J32"].astype(np.float64) - c["J64"]).max(axis=(2, 3)) > 1e-4
    s, i = (int(v) for v in np.argwhere((ts.sum(-1) == 2) & dis)[0])
    rows = [jh.quat_jvp_through(R[s, i], dR[s, i], int(k)).T for k in np.flatnonzero(ts[s, i])]
    assert np.abs(rows[0] - rows[1]).max() > 1e-3
    own = [np.abs(r - c["J64"][s, i, 3:]).max() < 1e-12 for r in rows]
    assert sorted(own) == [False, True]
    for r, is_own in zip(rows, own):
        B = c["J64"].copy(); B[s, i, 3:] = r
        assert len(jh.ajac_accept(B, c["q"], c["o"], J64=c["J64"])["quat"]) == 0
        assert len(jh.ajac_accept(B, c["q"], c["o"], J64=c["J64"], margin=0.0)["quat"]) == (0 if is_own else 1)
    B = c["J64"].copy(); B[s, i, 3:] = 0.5 * (rows[0] + rows[1])
    assert [tuple(v) for v in jh.ajac_accept(B, c["q"], c["o"], J64=c["J64"])["quat"]] == [(s, i)]


def test_panda_near_tie_rows(oracle_lib):
    """The deliberate near-tie rows: link 1 is tied (candidates 0 and 3) for |d| <= 3e-6 and untied at |d| = 1e-5 (gap 1.4e-5); at
    -pi/2 the two candidates are opposite quaternions."""
    m = model("panda_arm_no_gripper")
    o = oracle_lib.Oracle(m)
    q, ds = jh.panda_near_tie_q()
    H = o.fk(q.astype(np.float64), "f64")
    ts = jh.tie_set(H[:, 1, :3, :3])
    qa, cand = jh.quat_candidates(H[:, 1, :3, :3])
    inside = np.abs(ds) <= 3e-6
    assert np.array_equal(ts[inside], np.tile([True, False, False, True], (int(inside.sum()), 1)))
    assert (ts[~inside].sum(-1) == 1).all()
    gap = np.abs(qa[:, 0] - qa[:, 3])
    assert np.all(gap[~inside] > 1.3e-5) and np.all(gap[~inside] < 1.5e-5) and gap[inside].max() < 5e-6
    neg = q[:, 0] < 0
    assert np.abs(cand[neg, 0] + cand[neg, 3]).max() < 1e-5 and np.abs(cand[~neg, 0] - cand[~neg, 3]).max() < 1e-5
    J32 = o.analytic_jacobian(q, "f32")
    r = jh.ajac_accept(J32, q, o)
    assert len(r["pos"]) == 0 and len(r["quat"]) == 0


def test_quat_accept_sign_is_free_only_inside_a_tie(cases):
    c = cases["panda_arm_no_gripper"]
    R = c["H"][:, 5, :3, :3]
    qa, cand = jh.quat_candidates(R)
    quat = cand[np.arange(len(R)), qa.argmax(-1)]
    assert len(jh.quat_accept(quat, R)) == 0
    assert np.array_equal(jh.quat_accept(-quat, R), np.arange(len(R)))           # no tie in this batch: every negated row is refused
    bad = quat.copy(); bad[7, 2] += 2e-5
    assert np.array_equal(jh.quat_accept(bad, R), [7])
    # on a tie the other member's sign passes, and only there
    Rz = np.array([[[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])       # Rz(-pi/2): candidates 0 and 3 tied, opposite
    _, cz = jh.quat_candidates(Rz)
    assert len(jh.quat_accept(cz[:, 0], Rz)) == 0 and len(jh.quat_accept(cz[:, 3], Rz)) == 0 and np.abs(cz[0, 0] + cz[0, 3]).max() < 1e-15
    a = -np.pi / 2 + 1e-5                                                          # 1.4e-5 off the tie: outside the margin
    Ra = np.array([[[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]])
    _, ca = jh.quat_candidates(Ra)
    assert len(jh.quat_accept(ca[:, 0], Ra)) == 0 and len(jh.quat_accept(ca[:, 3], Ra)) == 1
    # the frame rule at the same rotation: trace = 1 > 0, the w branch alone
    assert len(jh.quat_accept(cz[:, 0], Rz, rule="frame")) == 0 and len(jh.quat_accept(cz[:, 3], Rz, rule="frame")) == 1


@pytest.mark.parametrize("D", jh.JTJ_WIDTHS)
def test_integer_case_is_exact_and_has_teeth(D):
    """jtj_int_case: exact in fp32 whatever the order; the bit comparison refuses a transposed-and-shifted pair, a row taken from the
    neighbouring sample, a padded column leaking in and a negative zero."""
    for n in jh.BATCHES:
        lin, ang, r, JtJ, Jtr = jh.jtj_int_case(n, D, seed=100 + D)
        J = np.concatenate([lin, ang], 1)
        acc = np.zeros((n, D, D), np.float32)
        for k in (5, 2, 0, 3, 1, 4):                                            # fp32 accumulation in another order
            acc = acc + J[:, k, :, None] * J[:, k, None, :]
        assert len(jh.int_mismatch(acc, JtJ)) == 0
        assert len(jh.int_mismatch((J * r[:, :, None]).sum(1, dtype=np.float32), Jtr)) == 0
    good = JtJ.astype(np.float32)
    if D >= 2:
        bad = good.copy()                                                       # (0, 1) and its transposed neighbour (1, 0 + 1)
        bad[:, 0, 1], bad[:, 1, 1] = good[:, 1, 1], good[:, 0, 1]
        assert len(jh.int_mismatch(bad, JtJ)) > 0
        bad = good.copy(); bad[:, 0, 1] = good[:, 0, 0]                          # an entry shifted by one column
        assert len(jh.int_mismatch(bad, JtJ)) > 0
        bad = good.copy(); bad[1:, D - 1] = good[:-1, D - 1]                     # a row shifted by one sample
        assert len(jh.int_mismatch(bad, JtJ)) > 0
    if 2 <= D < 8:                                                               # the 8-padded tile read with stride D
        pad = np.zeros((n, 8, 8), np.float32); pad[:, :D, :D] = good
        assert len(jh.int_mismatch(pad.reshape(n, 64)[:, :D * D].reshape(n, D, D).copy(), JtJ)) > 0
    z = np.flatnonzero(Jtr.reshape(-1) == 0)
    if len(z):
        bad = Jtr.astype(np.float32).reshape(-1); bad[z[0]] = np.float32(-0.0)
        assert len(jh.int_mismatch(bad.reshape(Jtr.shape), Jtr)) == 1


def test_cholesky_restated_bound():
    """k_jtj's Cholesky and triangular solves restated in numpy fp32 (chol_solve32), over every solve case of the GPU test: the largest
    residual / ((3 D + 1) 2^-24 scale) per width is
        D     1      2      3      4      5      6      7      8      9      13     16     22
        ratio 0.476  0.234  0.181  0.125  0.079  0.056  0.040  0.032  0.035  0.021  0.019  0.014
    (D = 1 is two roundings of one division each; the worst-case constant over-counts more as D grows).  The largest, 0.476, is what
    jacobian_helpers.CHOL_RATIO_MEASURED = 0.48 rounds up; the kernel's bound is CHOL_BOUND = 4 times that = 1.92 (3 D + 1) 2^-24
    of chol_residual's scale."""
    worst = {}
    for D in jh.JTJ_WIDTHS:
        for n in jh.BATCHES:
            lin, ang, r, J, JtJ, Jtr = jh.jtj_float_case(n, D, seed=200 + D)
            J32 = np.concatenate([lin, ang], 1)
            A32 = np.zeros((n, D, D), np.float32)
            b32 = np.zeros((n, D), np.float32)
            for k in range(6):
                A32 = jh._fma32(J32[:, k, :, None], J32[:, k, None, :], A32)
                b32 = jh._fma32(J32[:, k], r[:, k, None], b32)
            for lam in jh.solve_lambdas(n, seed=300 + D):
                dq = jh.chol_solve32(A32, b32, lam)
                assert np.isfinite(dq).all()
                res, scale = jh.chol_residual(JtJ, Jtr, lam, dq, J, r)
                worst[D] = max(worst.get(D, 0.0), float((res / ((3 * D + 1) * 2.0 ** -24 * scale)).max()))
                # the residual form has teeth: one component of dq off by 1e-3 of the largest is refused by the kernel's bound
                bad = dq.astype(np.float64); bad[0, D - 1] += 1e-3 * max(1.0, np.abs(bad[0]).max())
                res_b, scale_b = jh.chol_residual(JtJ, Jtr, lam, bad, J, r)
                assert res_b[0] > jh.chol_bound(D) * scale_b[0]
    print("largest residual / ((3 D + 1) 2^-24 scale) per width:", {D: round(v, 4) for D, v in worst.items()})
    top = max(worst.values())
    assert 0.5 * jh.CHOL_RATIO_MEASURED < top <= jh.CHOL_RATIO_MEASURED

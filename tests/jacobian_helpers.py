"""References for the three Jacobian entries (trk_fk_jacobian, trk_fk_analytic_jacobian, trk_jtj) in plain numpy fp64, restated from
oracle_impl.inc's quat_jvp / orc_rotmat_to_quat / frame_quat_wxyz, and the inputs the CPU and GPU tests share.

rotation_matrix_to_q (quaternion.py:135-166) forms four candidate quaternions and keeps the one with the largest q_abs; autograd
differentiates the KEPT one.  Two candidates are the same rotation, of either sign, and where their q_abs tie fp32 and fp64 may keep
different ones.  The rule here: a result must be what fp64 gives through SOME candidate whose q_abs is within `TIE_MARGIN` of the
largest -- where there is one such candidate it is the oracle's own, nothing is excluded and no share of blocks is waved through.

TIE_MARGIN = 4 TOL_H (TOL_H = 2e-6, DESIGN section 2's bound on an fp32 pose entry): each a_k is 1 +- three rotation entries, so
|delta a| <= 3 TOL_H; the largest q_abs = sqrt(a) is at least 1, so |delta q_abs| <= 1.5 TOL_H; two candidates can swap only within
3 TOL_H of each other, rounded up.  Frame.get_quaternion (frame.py:87-114, the geometric Jacobian's quaternion) chooses by the sign of
the trace and the largest diagonal entry instead: sums of three and differences of two entries, inside the same margin."""
import numpy as np

from torch_robotics_amd.kinmodel import JOINT_PRISMATIC

TOL_H = 2e-6
TIE_MARGIN = 4 * TOL_H
BATCHES = (1, 63, 65, 130)                 # one row, either side of a wavefront, two wavefronts and a tail
JTJ_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 22)

# Cholesky + two triangular solves of k_jtj, restated in numpy fp32 (chol_solve32), over every solve case: the largest
# residual / ((3 D + 1) 2^-24 scale) that test_jacobian_refs_cpu.py::test_cholesky_restated_bound measures (0.476, at D = 1), rounded
# up, and the bound the kernel is held to: 4 times that (the restatement differs in the rounding of 1 / ljj and in contraction only).
CHOL_RATIO_MEASURED = 0.48
CHOL_BOUND = 4 * CHOL_RATIO_MEASURED


# ---------------------------------------------------------------------------------------------------------------------------
# rotation_matrix_to_q and its JVP
# ---------------------------------------------------------------------------------------------------------------------------
def _numerators(M, one):
    """The four candidates' numerators (..., 4 candidates, 4 wxyz) of a matrix M (..., 3, 3); `one` = 1 for the matrix itself, 0 for a
    perturbation of it (the numerators are affine in the entries).  The diagonal slots hold a_k unmasked."""
    m00, m01, m02 = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    m10, m11, m12 = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    m20, m21, m22 = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    a = [one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22]
    rows = [[a[0], m21 - m12, m02 - m20, m10 - m01],
            [m21 - m12, a[1], m10 + m01, m02 + m20],
            [m02 - m20, m10 + m01, a[2], m12 + m21],
            [m10 - m01, m20 + m02, m21 + m12, a[3]]]
    return np.stack([np.stack(r, -1) for r in rows], -2), np.stack(a, -1)


def quat_candidates(R):
    """R (..., 3, 3) fp64 -> (qa (..., 4) = sqrt_with_mask(a_k), candidates (..., 4, 4): row k = candidate k as wxyz), denominators
    floored at 0.1 as the reference does."""
    R = np.asarray(R, np.float64)
    N, a = _numerators(R, 1.0)
    qa = np.where(a > 0, np.sqrt(np.maximum(a, 0.0)), 0.0)
    k = np.arange(4)
    N[..., k, k] = qa * qa                                   # the reference squares q_abs back (zero where a <= 0)
    return qa, N / (2.0 * np.maximum(qa, 0.1))[..., None]


def quat_jvp_through(R, dR, k):
    """d quat_wxyz (..., 4) of rotation_matrix_to_q at R (..., 3, 3) for the perturbation dR (..., 3, 3), differentiated THROUGH
    candidate k (an int, or an int array (...)): sqrt_with_mask has slope zero where a_k <= 0, the denominator 2 max(q_abs, 0.1) has
    slope zero below the floor."""
    R, dR = np.asarray(R, np.float64), np.asarray(dR, np.float64)
    R, dR = np.broadcast_arrays(R, dR)
    N, a = _numerators(R, 1.0)
    dN, da = _numerators(dR, 0.0)
    k = np.broadcast_to(np.asarray(k, np.int64), a.shape[:-1])[..., None]
    ak, dak = np.take_along_axis(a, k, -1)[..., 0], np.take_along_axis(da, k, -1)[..., 0]
    Nk = np.take_along_axis(N, k[..., None] + np.zeros((1, 4), np.int64), -2)[..., 0, :].copy()
    dNk = np.take_along_axis(dN, k[..., None] + np.zeros((1, 4), np.int64), -2)[..., 0, :].copy()
    pos = ak > 0
    ab, dab = np.where(pos, ak, 0.0), np.where(pos, dak, 0.0)
    qa = np.sqrt(ab)
    sel = np.arange(4) == k                                  # the candidate's own slot holds the masked a_k
    Nk = np.where(sel, ab[..., None], Nk)
    dNk = np.where(sel, dab[..., None], dNk)
    den = 2.0 * np.maximum(qa, 0.1)
    dden = np.where((qa > 0.1) & pos, dab / np.where(qa > 0, qa, 1.0), 0.0)
    return dNk / den[..., None] - Nk * (dden / (den * den))[..., None]


def tie_set(R, margin=TIE_MARGIN):
    """bool (..., 4): the candidates whose q_abs is within `margin` of the largest; a single True is the reference's own arg-max."""
    qa, _ = quat_candidates(R)
    return qa >= qa.max(-1, keepdims=True) - margin


def frame_tie_set(R, margin=TIE_MARGIN):
    """bool (..., 4): the branches Frame.get_quaternion (frame.py:87-114; oracle_impl.inc frame_quat_wxyz) can take within `margin`: w
    where the trace is positive, else the largest diagonal entry's component (the first of equal ones).  Branch k is the quaternion
    with component k positive, candidate k of quat_candidates."""
    R = np.asarray(R, np.float64)
    d = np.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]], -1)
    tr = d.sum(-1)
    out = np.zeros(R.shape[:-2] + (4,), bool)
    out[..., 0] = tr > -margin
    out[..., 1:] = (tr <= margin)[..., None] & (d >= d.max(-1, keepdims=True) - margin)
    return out


def frame_choice(R):
    """the branch frame_quat_wxyz takes in exact arithmetic (...,) int"""
    R = np.asarray(R, np.float64)
    d = np.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]], -1)
    i = np.zeros(d.shape[:-1], np.int64)
    i = np.where(d[..., 1] > d[..., 0], 1, i)
    i = np.where(d[..., 2] > np.take_along_axis(d, i[..., None], -1)[..., 0], 2, i)
    return np.where(d.sum(-1) > 0, 0, i + 1)


def rot_from_quat64(quat):
    """q_to_rotation_matrix (quaternion.py:102-120) of wxyz quaternions (n, 4) in fp64 -> (n, 3, 3): the rotation behind a quaternion
    the oracle returned without its matrix (the stateful walk's pose of orc_fk_jacobian)."""
    w, x, y, z = (np.asarray(quat, np.float64).reshape(-1, 4)[:, k] for k in range(4))
    dc = 2.0 / (w * w + x * x + y * y + z * z)
    return np.stack([1 - dc * (y * y + z * z), dc * (x * y - z * w), dc * (x * z + y * w),
                     dc * (x * y + z * w), 1 - dc * (x * x + z * z), dc * (y * z - x * w),
                     dc * (x * z - y * w), dc * (y * z + x * w), 1 - dc * (x * x + y * y)], -1).reshape(-1, 3, 3)


def quat_accept(quat_got, R64, margin=TIE_MARGIN, tol=5e-6, rule="argmax"):
    """A quaternion output (n, 4) wxyz against the fp64 rotations R64 (n, 3, 3): each row must be, within `tol`, a candidate of its
    rule's tie set -- rule 'argmax': rotation_matrix_to_q (tie_set), 'frame': Frame.get_quaternion (frame_tie_set).  Two candidates
    are +q and -q or the same quaternion, so the sign is free only inside a tie set.  -> the offending rows."""
    got = np.asarray(quat_got, np.float64).reshape(-1, 4)
    R64 = np.asarray(R64, np.float64).reshape(-1, 3, 3)
    assert len(got) == len(R64)
    _, cand = quat_candidates(R64)
    ts = tie_set(R64, margin) if rule == "argmax" else frame_tie_set(R64, margin)
    ok = (np.abs(cand - got[:, None, :]).max(-1) <= tol) & ts
    return np.flatnonzero(~ok.any(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# the analytic Jacobian of every link
# ---------------------------------------------------------------------------------------------------------------------------
def chain_mask(model):
    """bool (L, D): DOF d is a joint on the path root..link i"""
    L, D = model.n_links, model.n_dofs
    out = np.zeros((L, D), bool)
    for i in range(L):
        j = i
        while j > 0:
            if int(model.dof_idx[j]) >= 0:
                out[i, int(model.dof_idx[j])] = True
            j = int(model.parent[j])
    return out


def pass_mask(model, q):
    """bool (n, D): the stateless FK's clamp mask per DOF (rigid_body.py:157-160; oracle_impl.inc joint_pose): the gradient passes
    unless the joint is clamped and q lies outside [lower, upper] -- a q exactly on a limit passes."""
    q = np.asarray(q, np.float64).reshape(-1, model.n_dofs)
    out = np.ones(q.shape, bool)
    for j in range(1, model.n_links):
        d = int(model.dof_idx[j])
        if d >= 0 and int(model.clamp[j]):
            out[:, d] = (q[:, d] >= float(model.lower[j])) & (q[:, d] <= float(model.upper[j]))
    return out


def rotation_perturbations(model, q, H64):
    """dR (n, L, D, 3, 3) fp64: d R_i / d q_d = [w_d]x R_i for the revolute joints on link i's path, w_d = pass * sign * the joint's axis
    in the world, zero elsewhere (prismatic, clamped and off-path joints) -- from the oracle's fp64 FK H64 (n, L, 4, 4) and the pass
    mask, as orc_fk_analytic_jacobian forms it."""
    n, L, D = H64.shape[0], model.n_links, model.n_dofs
    Rw = H64[..., :3, :3]
    ps, on = pass_mask(model, q), chain_mask(model)
    dR = np.zeros((n, L, D, 3, 3))
    for j in range(1, L):
        d, jt = int(model.dof_idx[j]), int(model.joint_type[j])
        if d < 0 or jt == JOINT_PRISMATIC:
            continue
        w = float(model.rot_sign[j]) * Rw[:, j, :, int(model.rot_axis[j])] * ps[:, d, None]        # (n, 3)
        for i in np.flatnonzero(on[:, d]):
            dR[:, i, d] = np.cross(w[:, None, :], Rw[:, i].transpose(0, 2, 1)).transpose(0, 2, 1)      # column c: w x R_i[:, c]
    return dR


def ajac_accept(J_got, q, oracle, margin=TIE_MARGIN, pos_tol=3e-6, quat_tol=5e-6, J64=None, H64=None):
    """J_got (n, L, 7, D) against the fp64 oracle at q (the fp32 values, evaluated exactly).  For EVERY (sample, link): the three
    position rows within pos_tol * max(1, largest |link translation|) of the oracle's; the four quaternion rows within quat_tol of the
    fp64 JVP through SOME member of the link's tie set (one member: the oracle's own choice).  -> dict(pos, quat: offending (sample, link)
    index arrays (k, 2); tied: bool (n, L), blocks with more than one member)."""
    m = oracle.model
    q64 = np.asarray(q, np.float32).astype(np.float64).reshape(-1, m.n_dofs)
    J_got = np.asarray(J_got, np.float64)
    if H64 is None:                                   # (J64, H64: the oracle's results at q where the caller has them already)
        H64 = oracle.fk(q64, "f64")
    if J64 is None:
        J64 = oracle.analytic_jacobian(q64, "f64")
    assert J_got.shape == J64.shape, (J_got.shape, J64.shape)
    scale = max(1.0, float(np.abs(H64[..., :3, 3]).max()))
    pos_bad = np.abs(J_got[:, :, :3] - J64[:, :, :3]).max(axis=(2, 3)) > pos_tol * scale
    Rw = H64[..., :3, :3]
    dR = rotation_perturbations(m, q64, H64)
    ts = tie_set(Rw, margin)                                                       # (n, L, 4)
    got_q = J_got[:, :, 3:].transpose(0, 1, 3, 2)                                  # (n, L, D, 4)
    ok = np.zeros(ts.shape[:2], bool)
    for k in range(4):
        if ts[..., k].any():
            jvp = quat_jvp_through(Rw[:, :, None], dR, k)                          # (n, L, D, 4)
            ok |= ts[..., k] & (np.abs(jvp - got_q).max(axis=(2, 3)) <= quat_tol)
    return dict(pos=np.argwhere(pos_bad), quat=np.argwhere(~ok), tied=ts.sum(-1) > 1)


def jacobian_inputs(model, seed=5, n=130):
    """The q of the GPU Jacobian tests (n + 4, D) fp32: n rows uniform(-3, 3) -- beyond most limits, so the stateful walk's clamps and the
    stateless walk's masks are exercised -- and four rows with one limited joint exactly at its lower limit and another at its upper."""
    D = model.n_dofs
    rng = np.random.default_rng(seed)
    q = rng.uniform(-3.0, 3.0, (n, D)).astype(np.float32)
    lim = [j for j in range(1, model.n_links) if int(model.dof_idx[j]) >= 0 and int(model.has_limits[j])]
    extra = 0.3 * q[:4].copy()
    for r in range(4):
        if lim:
            a, b = lim[r % len(lim)], lim[(r + 1 + len(lim) // 2) % len(lim)]
            extra[r, int(model.dof_idx[a])] = np.float32(model.lower[a])
            extra[r, int(model.dof_idx[b])] = np.float32(model.upper[b])
    return np.concatenate([q, extra]).astype(np.float32)


def batch_rows(n_total):
    """{batch size: rows of jacobian_inputs} for BATCHES: prefixes, and the last 130 rows (the limit rows among them)"""
    return {b: (np.arange(b) if b < 130 else np.arange(n_total - 130, n_total)) for b in BATCHES}


MOVED_BASE = [0.1234, -0.2345, 0.0567, 0.9659258, 0.0, 0.0, 0.2588190]       # xyz + wxyz, as KinModel.set_base_pose


def panda_near_tie_q():
    """(18, 7) fp32: q1 = +-pi/2 + d, the other joints 0.  Link 1's rotation is Rz(q1): a_0 = 2 + 2 cos q1 and a_3 = 2 - 2 cos q1 tie at
    cos q1 = 0, their q_abs differ by 1.414 |d|.  At -pi/2 the two candidates are +q and -q; at +pi/2 they are the same quaternion."""
    ds = [0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-6, -3e-6, 1e-5, -1e-5]
    q = np.zeros((2 * len(ds), 7), np.float32)
    q[:, 0] = np.float32([s * np.pi / 2 + d for s in (-1.0, 1.0) for d in ds])
    return q, np.array(ds + ds)


# ---------------------------------------------------------------------------------------------------------------------------
# the normal equations
# ---------------------------------------------------------------------------------------------------------------------------
def jtj_int_case(n, D, seed):
    """Integer-valued fp32 lin, ang (n, 3, D) and r (n, 6) in [-15, 15] with their exact int64 JtJ (n, D, D) and Jtr (n, D).  A product
    is at most 225 and a 6-term sum at most 1350 in magnitude: every partial sum is an integer below 2^24, so fp32 gives it exactly in
    any order, fused or not, MFMA included -- the result has one right answer, to the bit.
    Sample 0 is six signed copies of one row of distinct non-zero values c: its JtJ = 6 c c^T has no two equal neighbours, so entry
    (i, j) differs from (i, j +- 1), (i +- 1, j) and from (j, i +- 1) in that sample whatever the others hold (asserted below)."""
    rng = np.random.default_rng(seed)
    J = rng.integers(-15, 16, (n, 6, D))
    r = rng.integers(-15, 16, (n, 6))
    vals = np.concatenate([np.arange(-15, 0), np.arange(1, 16)])
    J[0] = rng.permutation(vals)[:D][None, :] * rng.choice([-1, 1], 6)[:, None]
    JtJ = np.einsum("nki,nkj->nij", J, J).astype(np.int64)
    Jtr = np.einsum("nki,nk->ni", J, r).astype(np.int64)
    assert np.abs(JtJ).max() <= 1350 and np.abs(Jtr).max() <= 1350
    for i in range(D):
        for j in range(D):
            for a, b in ((i, j + 1), (i, j - 1), (i + 1, j), (i - 1, j), (j, i + 1), (j, i - 1)):
                if 0 <= a < D and 0 <= b < D and (a, b) != (i, j) and (a, b) != (j, i):
                    assert (JtJ[:, i, j] != JtJ[:, a, b]).any(), (D, i, j, a, b)
    J32 = J.astype(np.float32)
    return np.ascontiguousarray(J32[:, :3]), np.ascontiguousarray(J32[:, 3:]), r.astype(np.float32), JtJ, Jtr


def int_mismatch(got, ref_int):
    """indices where an fp32 result is not the exact integer (bit comparison: -0.0 for 0 is refused as well)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref_int.shape, (got.dtype, got.shape, ref_int.shape)
    return np.argwhere(got.view(np.int32) != ref_int.astype(np.float32).view(np.int32))


def jtj_float_case(n, D, seed):
    """random-normal lin, ang (n, 3, D), r (n, 6) fp32 and their fp64 J (n, 6, D), JtJ, Jtr"""
    rng = np.random.default_rng(seed)
    lin, ang = rng.standard_normal((n, 3, D)).astype(np.float32), rng.standard_normal((n, 3, D)).astype(np.float32)
    r = rng.standard_normal((n, 6)).astype(np.float32)
    J = np.concatenate([lin, ang], 1).astype(np.float64)
    return lin, ang, r, J, np.einsum("nki,nkj->nij", J, J), np.einsum("nki,nk->ni", J, r.astype(np.float64))


def solve_lambdas(n, seed):
    """the dampings of the solve cases: 1e-2, 1, and one per sample in [1e-2, 1] -- fp32 arrays of 1, 1 and n values"""
    per = np.random.default_rng(seed).uniform(1e-2, 1.0, n).astype(np.float32)
    return [np.float32([1e-2]), np.float32([1.0]), per]


def chol_residual(JtJ64, Jtr64, lam, dq, J64, r64):
    """Per sample: the fp64 residual |(JtJ + lam I) dq - Jtr|_inf and the scale (| |J|^T |J| |_inf + lam) |dq|_inf + | |J|^T |r| |_inf
    it is measured in (Higham's backward-error form: forming JtJ and Jtr in fp32, the factorisation and the two solves each perturb
    by a multiple of the unit roundoff times these)."""
    n, D = Jtr64.shape
    lam = np.broadcast_to(np.asarray(lam, np.float64).reshape(-1), (n,))
    dq = np.asarray(dq, np.float64)
    res = np.abs(np.einsum("nij,nj->ni", JtJ64, dq) + lam[:, None] * dq - Jtr64).max(-1)
    aJ, ar = np.abs(J64), np.abs(np.asarray(r64, np.float64))
    nA = np.einsum("nki,nkj->nij", aJ, aJ).sum(-1).max(-1)
    nb = np.einsum("nki,nk->ni", aJ, ar).max(-1)
    return res, (nA + lam) * np.abs(dq).max(-1) + nb


def chol_bound(D):
    """the residual the kernel's solve may leave, per unit of chol_residual's scale"""
    return CHOL_BOUND * (3 * D + 1) * 2.0 ** -24


def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays: the product of two fp32 values is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chol_solve32(JtJ32, Jtr32, lam32):
    """k_jtj's in-place Cholesky of JtJ + lam I and its two triangular solves, restated in numpy fp32 in the kernel's fmaf order:
    JtJ32 (n, D, D), Jtr32 (n, D), lam32 (1,) or (n,) -> dq (n, D) fp32."""
    A = np.array(JtJ32, np.float32)
    b = np.array(Jtr32, np.float32)
    n, D = b.shape
    lam = np.broadcast_to(np.asarray(lam32, np.float32).reshape(-1), (n,))
    for j in range(D):
        s = (A[:, j, j] + lam).astype(np.float32)
        for k in range(j):
            s = _fma32(-A[:, j, k], A[:, j, k], s)
        ljj = np.sqrt(np.maximum(s, np.float32(1e-20))).astype(np.float32)
        inv = (np.float32(1.0) / ljj).astype(np.float32)
        A[:, j, j] = ljj
        for i in range(j + 1, D):
            v = A[:, i, j]
            for k in range(j):
                v = _fma32(-A[:, i, k], A[:, j, k], v)
            A[:, i, j] = (v * inv).astype(np.float32)
    for i in range(D):
        v = b[:, i]
        for k in range(i):
            v = _fma32(-A[:, i, k], b[:, k], v)
        b[:, i] = (v / A[:, i, i]).astype(np.float32)
    for i in range(D - 1, -1, -1):
        v = b[:, i]
        for k in range(i + 1, D):
            v = _fma32(-A[:, k, i], b[:, k], v)
        b[:, i] = (v / A[:, i, i]).astype(np.float32)
    return b

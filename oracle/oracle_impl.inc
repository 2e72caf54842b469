/*
 * oracle_impl.inc -- TEST INFRASTRUCTURE (CPU restatement of the reference algorithm).
 * Included twice by oracle.c with REAL = float / double and FN(x) = x_f32 / x_f64.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may call this.
 * The product (torch_robotics_amd/, libtrk.so) never links or loads it.
 *
 * Every function cites the reference lines it restates (paths relative to
 * /root/reference/torch_robotics/).  Parity of this file is pinned by tests/test_oracle_golden.py
 * against vectors produced by the reference itself (oracle/gen_golden.py).
 */

typedef struct { REAL R[9]; REAL t[3]; } FN(Pose);

static inline void FN(mat3_mul)(const REAL* A, const REAL* B, REAL* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
static inline void FN(mat3_vec)(const REAL* A, const REAL* v, REAL* o) {
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
static inline void FN(mat3T_vec)(const REAL* A, const REAL* v, REAL* o) {
    for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
/* geometrics/utils.py:11-17 multiply_transform: w_R_c = w_R_l @ l_R_c ; w_t_c = w_R_l @ l_t_c + w_t_l */
static inline void FN(pose_mul)(const FN(Pose)* a, const FN(Pose)* b, FN(Pose)* o) {
    FN(Pose) r;
    FN(mat3_mul)(a->R, b->R, r.R);
    FN(mat3_vec)(a->R, b->t, r.t);
    for (int k = 0; k < 3; ++k) r.t[k] += a->t[k];
    *o = r;
}
/* spatial_vector.py:8-47 x_rot / y_rot / z_rot */
static inline void FN(axis_rot)(int axis, REAL ang, REAL* R) {
    REAL c = COS(ang), s = SIN(ang);
    for (int k = 0; k < 9; ++k) R[k] = 0;
    if (axis == 0)      { R[0] = 1; R[4] = c; R[5] = -s; R[7] = s; R[8] = c; }
    else if (axis == 1) { R[0] = c; R[2] = s; R[4] = 1; R[6] = -s; R[8] = c; }
    else                { R[0] = c; R[1] = -s; R[3] = s; R[4] = c; R[8] = 1; }
}
/* d/d(angle) of the above */
static inline void FN(axis_rot_d)(int axis, REAL ang, REAL* R) {
    REAL c = COS(ang), s = SIN(ang);
    for (int k = 0; k < 9; ++k) R[k] = 0;
    if (axis == 0)      { R[4] = -s; R[5] = -c; R[7] = c; R[8] = -s; }
    else if (axis == 1) { R[0] = -s; R[2] = c; R[6] = -c; R[8] = -s; }
    else                { R[0] = -s; R[1] = -c; R[3] = c; R[4] = -s; }
}

/* rigid_body.py:153-190: local joint transform of link i for the stateless path.
 * Returns the clamp mask (1 = gradient passes). */
static inline int FN(joint_pose)(const TrkKinModelDesc* m, int i, const REAL* q, FN(Pose)* out, REAL* qhat_out) {
    const float* Rf = m->R_fixed + 9 * i;
    int jt = m->joint_type[i];
    int pass = 1;
    REAL qh = 0;
    if (jt != TRK_JOINT_FIXED) {
        qh = q[m->dof_idx[i]];
        if (m->clamp[i]) {                              /* :157-160 torch.clamp(q, lower, upper) */
            REAL lo = (REAL)m->lower[i], hi = (REAL)m->upper[i];
            pass = (qh >= lo) && (qh <= hi);
            qh = qh < lo ? lo : (qh > hi ? hi : qh);
        }
    }
    if (qhat_out) *qhat_out = qh;
    if (jt == TRK_JOINT_REVOLUTE || jt == TRK_JOINT_CONTINUOUS) {   /* :162-174 */
        REAL rot[9], Rf_[9];
        for (int k = 0; k < 9; ++k) Rf_[k] = (REAL)Rf[k];
        FN(axis_rot)(m->rot_axis[i], (REAL)m->rot_sign[i] * qh, rot);
        FN(mat3_mul)(Rf_, rot, out->R);
        for (int k = 0; k < 3; ++k) out->t[k] = (REAL)m->trans[3 * i + k];
    } else if (jt == TRK_JOINT_PRISMATIC) {             /* :175-182, axis NOT rotated by R_fixed */
        for (int k = 0; k < 9; ++k) out->R[k] = (REAL)Rf[k];
        for (int k = 0; k < 3; ++k) out->t[k] = (REAL)m->trans[3 * i + k] + (REAL)m->axis[3 * i + k] * qh;
    } else {                                            /* fixed :186-190 */
        for (int k = 0; k < 9; ++k) out->R[k] = (REAL)Rf[k];
        for (int k = 0; k < 3; ++k) out->t[k] = (REAL)m->trans[3 * i + k];
    }
    return pass;
}

static inline void FN(base_pose)(const TrkKinModelDesc* m, FN(Pose)* b) {
    for (int k = 0; k < 9; ++k) b->R[k] = (REAL)m->base_R[k];
    for (int k = 0; k < 3; ++k) b->t[k] = (REAL)m->base_t[k];
}

static inline void FN(pose_to_H)(const FN(Pose)* p, REAL* H) {    /* frame.py:81-85 */
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) H[4 * r + c] = p->R[3 * r + c];
        H[4 * r + 3] = p->t[r];
    }
    H[12] = 0; H[13] = 0; H[14] = 0; H[15] = 1;
}

/* World poses of all links for one sample, left-to-right chain walk:
 * pose_i = pose_parent(i) o joint_pose_i   (same value as rigid_body.py:200-211 up to fp association) */
static void FN(fk_sample)(const TrkKinModelDesc* m, const REAL* q, FN(Pose)* world, FN(Pose)* local, int* pass) {
    int L = m->n_links;
    for (int p = 0; p < L; ++p) {
        int i = m->order[p];
        if (i == 0) {                                   /* root: base pose (rigid_body.py:202-208) */
            FN(base_pose)(m, &world[0]);
            if (local) local[0] = world[0];
            if (pass) pass[0] = 1;
            continue;
        }
        FN(Pose) jp;
        int ps = FN(joint_pose)(m, i, q, &jp, NULL);
        if (local) local[i] = jp;
        if (pass) pass[i] = ps;
        FN(pose_mul)(&world[m->parent[i]], &jp, &world[i]);
    }
}

/* robot_tree.py:267-301 compute_forward_kinematics_all_links -> H [N,L,4,4] (chain-walk association) */
void FN(orc_fk)(const TrkKinModelDesc* m, const REAL* q, int64_t n, REAL* H) {
    int L = m->n_links, D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        FN(fk_sample)(m, q + s * D, world, NULL, NULL);
        for (int i = 0; i < L; ++i) FN(pose_to_H)(&world[i], H + (s * L + i) * 16);
    }
}

/* Same op with the reference's own association order: every link's pose is built right-to-left,
 * T_a1 o (T_a2 o (... o T_ak)), then pre-multiplied by the root/base pose (rigid_body.py:195-211).
 * O(L * depth) composes per sample, like the reference. */
void FN(orc_fk_ref_order)(const TrkKinModelDesc* m, const REAL* q, int64_t n, REAL* H) {
    int L = m->n_links, D = m->n_dofs;
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) local[TRK_MAX_LINKS], base;
        FN(base_pose)(m, &base);
        for (int i = 1; i < L; ++i) FN(joint_pose)(m, i, q + s * D, &local[i], NULL);
        for (int i = 0; i < L; ++i) {
            FN(Pose) acc;
            if (i == 0) { acc = base; }
            else {
                acc = local[i];
                for (int a = m->parent[i]; a > 0; a = m->parent[a]) FN(pose_mul)(&local[a], &acc, &acc);
                FN(pose_mul)(&base, &acc, &acc);
            }
            FN(pose_to_H)(&acc, H + (s * L + i) * 16);
        }
    }
}

/* Reverse mode of orc_fk: gH [N,L,4,4] -> gq [N,D] (SURVEY.md Appendix B "FK backward", matrix-adjoint
 * form; equals autograd through rigid_body.py:146-211 incl. the zero gradient of torch.clamp outside
 * the limits :157-160). */
static void FN(fk_backward_sample)(const TrkKinModelDesc* m, const REAL* q, const REAL* gH, REAL* gq) {
    int L = m->n_links, D = m->n_dofs;
    FN(Pose) world[TRK_MAX_LINKS], local[TRK_MAX_LINKS];
    int pass[TRK_MAX_LINKS];
    REAL Rb[TRK_MAX_LINKS][9], tb[TRK_MAX_LINKS][3];
    FN(fk_sample)(m, q, world, local, pass);
    for (int i = 0; i < L; ++i) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rb[i][3 * r + c] = gH[i * 16 + 4 * r + c];
            tb[i][r] = gH[i * 16 + 4 * r + 3];
        }
    }
    for (int d = 0; d < D; ++d) gq[d] = 0;
    for (int p = L - 1; p >= 1; --p) {
        int i = m->order[p], par = m->parent[i];
        const REAL* Rp = world[par].R;
        const REAL* Rl = local[i].R; const REAL* tl = local[i].t;
        /* R_i = R_p R_loc ; t_i = R_p t_loc + t_p */
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                REAL acc = 0;
                for (int k = 0; k < 3; ++k) acc += Rb[i][3 * r + k] * Rl[3 * c + k];     /* Rbar_i R_loc^T */
                Rb[par][3 * r + c] += acc + tb[i][r] * tl[c];                             /* + tbar_i t_loc^T */
            }
        for (int k = 0; k < 3; ++k) tb[par][k] += tb[i][k];
        int jt = m->joint_type[i];
        if (jt == TRK_JOINT_FIXED) continue;
        REAL g = 0, qh;
        FN(Pose) tmp;
        FN(joint_pose)(m, i, q, &tmp, &qh);
        if (jt == TRK_JOINT_PRISMATIC) {
            REAL tl_b[3];
            FN(mat3T_vec)(Rp, tb[i], tl_b);                       /* tbar_loc = R_p^T tbar_i */
            for (int k = 0; k < 3; ++k) g += (REAL)m->axis[3 * i + k] * tl_b[k];
        } else {
            REAL Rlb[9], A[9], dR[9], Rf[9];
            for (int r = 0; r < 3; ++r)                           /* Rbar_loc = R_p^T Rbar_i */
                for (int c = 0; c < 3; ++c) {
                    REAL acc = 0;
                    for (int k = 0; k < 3; ++k) acc += Rp[3 * k + r] * Rb[i][3 * k + c];
                    Rlb[3 * r + c] = acc;
                }
            for (int k = 0; k < 9; ++k) Rf[k] = (REAL)m->R_fixed[9 * i + k];
            for (int r = 0; r < 3; ++r)                           /* A = R_f^T Rbar_loc */
                for (int c = 0; c < 3; ++c) {
                    REAL acc = 0;
                    for (int k = 0; k < 3; ++k) acc += Rf[3 * k + r] * Rlb[3 * k + c];
                    A[3 * r + c] = acc;
                }
            REAL sg = (REAL)m->rot_sign[i];
            FN(axis_rot_d)(m->rot_axis[i], sg * qh, dR);
            for (int k = 0; k < 9; ++k) g += A[k] * dR[k];
            g *= sg;
        }
        if (!pass[i]) g = 0;
        gq[m->dof_idx[i]] += g;
    }
}

void FN(orc_fk_backward)(const TrkKinModelDesc* m, const REAL* q, const REAL* gH, int64_t n, REAL* gq) {
    int L = m->n_links, D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) FN(fk_backward_sample)(m, q + s * D, gH + s * L * 16, gq + s * D);
}

/* frame.py:87-114 Frame.get_quaternion (xyzw) followed by q_convert_wxyz quaternion.py:240-242 */
static void FN(frame_quat_wxyz)(const REAL* R, REAL* out) {
    REAL M[4][4] = {{R[0], R[1], R[2], 0}, {R[3], R[4], R[5], 0}, {R[6], R[7], R[8], 0}, {0, 0, 0, 1}};
    REAL t = M[0][0] + M[1][1] + M[2][2] + M[3][3], q[4];
    if (t > M[3][3]) {
        q[3] = t; q[2] = M[1][0] - M[0][1]; q[1] = M[0][2] - M[2][0]; q[0] = M[2][1] - M[1][2];
    } else {
        int i = 0, j = 1, k = 2;
        if (M[1][1] > M[0][0]) { i = 1; j = 2; k = 0; }
        if (M[2][2] > M[i][i]) { i = 2; j = 0; k = 1; }
        t = M[i][i] - (M[j][j] + M[k][k]) + M[3][3];
        q[i] = t; q[j] = M[i][j] + M[j][i]; q[k] = M[k][i] + M[i][k]; q[3] = M[k][j] - M[j][k];
    }
    REAL sc = (REAL)0.5 / SQRT(t * M[3][3]);
    out[0] = q[3] * sc; out[1] = q[0] * sc; out[2] = q[1] * sc; out[3] = q[2] * sc;
}

/* robot_tree.py:136-190 update_kinematic_state + :218-248 geometric Jacobian, for link `link`.
 * Stateful-path quirks kept: rotation about sf_rot_axis with the axis sign ignored (rigid_body.py:226-227),
 * clamp whenever limits exist (:218-219), Jacobian columns only for controlled links idx with
 * (idx-1) <= joint_list_idx[link] (:239-240), joint axis = column jac_axis of the world rotation (:242-244). */
void FN(orc_fk_jacobian)(const TrkKinModelDesc* m, const REAL* q, const REAL* qd, int64_t n, int link,
                         REAL* pos, REAL* quat, REAL* lin_jac, REAL* ang_jac, REAL* vel_lin, REAL* vel_ang) {
    int L = m->n_links, D = m->n_dofs;
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        REAL vl[TRK_MAX_LINKS][3], va[TRK_MAX_LINKS][3];
        const REAL* qs = q + s * D;
        for (int p = 0; p < L; ++p) {
            int i = m->order[p];
            if (i == 0) { FN(base_pose)(m, &world[0]); for (int k = 0; k < 3; ++k) vl[0][k] = va[0][k] = 0; continue; }
            FN(Pose) jp;
            int jt = m->joint_type[i];
            REAL qh = 0, qdv = 0;
            if (jt != TRK_JOINT_FIXED) {
                qh = qs[m->dof_idx[i]];
                if (qd) qdv = qd[s * D + m->dof_idx[i]];
                if (m->sf_clamp[i]) {
                    REAL lo = (REAL)m->lower[i], hi = (REAL)m->upper[i];
                    qh = qh < lo ? lo : (qh > hi ? hi : qh);
                }
            }
            for (int k = 0; k < 3; ++k) jp.t[k] = (REAL)m->trans[3 * i + k];
            REAL Rf[9];
            for (int k = 0; k < 9; ++k) Rf[k] = (REAL)m->R_fixed[9 * i + k];
            if (jt == TRK_JOINT_REVOLUTE || jt == TRK_JOINT_CONTINUOUS) {
                REAL rot[9];
                FN(axis_rot)(m->sf_rot_axis[i], qh, rot);
                FN(mat3_mul)(Rf, rot, jp.R);
            } else {
                for (int k = 0; k < 9; ++k) jp.R[k] = Rf[k];
                if (jt == TRK_JOINT_PRISMATIC)
                    for (int k = 0; k < 3; ++k) jp.t[k] += (REAL)m->axis[3 * i + k] * qh;
            }
            int par = m->parent[i];
            FN(pose_mul)(&world[par], &jp, &world[i]);
            /* velocities: parentToChild = inverse(joint_pose) (frame.py:57-62);
             * MotionVec.transform spatial_vector.py:87-97: ang' = R a ; lin' = (skew(t) R) a + R l ;
             * joint_vel = (lin 0, ang qd*axis) rigid_body.py:253-256 */
            REAL Rt[9], tinv[3], tmp[3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rt[3 * r + c] = jp.R[3 * c + r];
            FN(mat3_vec)(Rt, jp.t, tmp);
            for (int k = 0; k < 3; ++k) tinv[k] = -tmp[k];
            REAL na[3], nl[3], Ra[3];
            FN(mat3_vec)(Rt, va[par], na);
            FN(mat3_vec)(Rt, va[par], Ra);
            nl[0] = tinv[1] * Ra[2] - tinv[2] * Ra[1];
            nl[1] = tinv[2] * Ra[0] - tinv[0] * Ra[2];
            nl[2] = tinv[0] * Ra[1] - tinv[1] * Ra[0];
            FN(mat3_vec)(Rt, vl[par], tmp);
            for (int k = 0; k < 3; ++k) {
                vl[i][k] = nl[k] + tmp[k];
                va[i][k] = na[k] + qdv * (REAL)m->axis[3 * i + k];
            }
        }
        for (int k = 0; k < 3; ++k) pos[s * 3 + k] = world[link].t[k];
        FN(frame_quat_wxyz)(world[link].R, quat + s * 4);
        if (vel_lin) for (int k = 0; k < 3; ++k) vel_lin[s * 3 + k] = vl[link][k];
        if (vel_ang) for (int k = 0; k < 3; ++k) vel_ang[s * 3 + k] = va[link][k];
        for (int k = 0; k < 3 * D; ++k) { lin_jac[s * 3 * D + k] = 0; ang_jac[s * 3 * D + k] = 0; }
        int pj = m->joint_list_idx[link];
        for (int i = 1; i < L; ++i) {
            int d = m->dof_idx[i];
            if (d < 0) continue;
            if ((i - 1) > pj) continue;
            int ax = m->jac_axis[i];
            if (ax < 0) continue;
            const REAL* R = world[i].R; const REAL* p = world[i].t;
            REAL z[3] = {R[ax], R[3 + ax], R[6 + ax]};
            REAL r[3] = {world[link].t[0] - p[0], world[link].t[1] - p[1], world[link].t[2] - p[2]};
            REAL c[3] = {z[1] * r[2] - z[2] * r[1], z[2] * r[0] - z[0] * r[2], z[0] * r[1] - z[1] * r[0]};
            for (int k = 0; k < 3; ++k) { lin_jac[(s * 3 + k) * D + d] = c[k]; ang_jac[(s * 3 + k) * D + d] = z[k]; }
        }
    }
}

/* d quat_wxyz for a rotation perturbation dR, differentiating rotation_matrix_to_q (quaternion.py:135-166) the way
 * autograd does: through the SELECTED candidate (arg-max of q_abs), sqrt_with_mask (zero slope where the argument
 * is <= 0) and the 0.1 floor of the denominator. */
static void FN(quat_jvp)(const REAL* m, const REAL* dm, REAL* dq) {
    REAL a[4] = {1 + m[0] + m[4] + m[8], 1 + m[0] - m[4] - m[8], 1 - m[0] + m[4] - m[8], 1 - m[0] - m[4] + m[8]};
    REAL da[4] = {dm[0] + dm[4] + dm[8], dm[0] - dm[4] - dm[8], -dm[0] + dm[4] - dm[8], -dm[0] - dm[4] + dm[8]};
    REAL qa[4];
    int b = 0;
    for (int k = 0; k < 4; ++k) qa[k] = a[k] > 0 ? SQRT(a[k]) : 0;
    for (int k = 1; k < 4; ++k) if (qa[k] > qa[b]) b = k;
    const REAL ab = a[b] > 0 ? a[b] : 0, dab = a[b] > 0 ? da[b] : 0;
    REAL N[4], dN[4];
    if (b == 0)      { N[0] = ab; N[1] = m[7] - m[5]; N[2] = m[2] - m[6]; N[3] = m[3] - m[1];
                       dN[0] = dab; dN[1] = dm[7] - dm[5]; dN[2] = dm[2] - dm[6]; dN[3] = dm[3] - dm[1]; }
    else if (b == 1) { N[0] = m[7] - m[5]; N[1] = ab; N[2] = m[3] + m[1]; N[3] = m[2] + m[6];
                       dN[0] = dm[7] - dm[5]; dN[1] = dab; dN[2] = dm[3] + dm[1]; dN[3] = dm[2] + dm[6]; }
    else if (b == 2) { N[0] = m[2] - m[6]; N[1] = m[3] + m[1]; N[2] = ab; N[3] = m[5] + m[7];
                       dN[0] = dm[2] - dm[6]; dN[1] = dm[3] + dm[1]; dN[2] = dab; dN[3] = dm[5] + dm[7]; }
    else             { N[0] = m[3] - m[1]; N[1] = m[6] + m[2]; N[2] = m[7] + m[5]; N[3] = ab;
                       dN[0] = dm[3] - dm[1]; dN[1] = dm[6] + dm[2]; dN[2] = dm[7] + dm[5]; dN[3] = dab; }
    const REAL den = 2 * (qa[b] > (REAL)0.1 ? qa[b] : (REAL)0.1);
    const REAL dden = (qa[b] > (REAL)0.1 && a[b] > 0) ? dab / qa[b] : 0;      /* 2 * d sqrt(a) = da / sqrt(a) */
    for (int k = 0; k < 4; ++k) dq[k] = dN[k] / den - N[k] * dden / (den * den);
}

/* robot_tree.py:250-265 compute_analytical_jacobian_all_links: J [N, L, 7, D] = d [pos(3), quat_wxyz(4)] / d q of
 * every link, i.e. autograd through the stateless FK (clamp mask, axis sign) and rotation_matrix_to_q. */
void FN(orc_fk_analytic_jacobian)(const TrkKinModelDesc* m, const REAL* q, int64_t n, REAL* J) {
    int L = m->n_links, D = m->n_dofs;
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        int pass[TRK_MAX_LINKS];
        FN(fk_sample)(m, q + s * D, world, NULL, pass);
        REAL* Js = J + s * L * 7 * D;
        for (int k = 0; k < L * 7 * D; ++k) Js[k] = 0;
        for (int i = 1; i < L; ++i) {
            for (int j = i; j > 0; j = m->parent[j]) {              /* joints on the path root..i */
                int jt = m->joint_type[j];
                if (jt == TRK_JOINT_FIXED) continue;
                int d = m->dof_idx[j];
                REAL dp[3] = {0, 0, 0}, dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (pass[j]) {
                    if (jt == TRK_JOINT_PRISMATIC) {
                        REAL ax[3] = {(REAL)m->axis[3 * j], (REAL)m->axis[3 * j + 1], (REAL)m->axis[3 * j + 2]};
                        FN(mat3_vec)(world[m->parent[j]].R, ax, dp);
                    } else {
                        int ax = m->rot_axis[j];
                        REAL sg = (REAL)m->rot_sign[j];
                        const REAL* Rj = world[j].R;
                        REAL w[3] = {sg * Rj[ax], sg * Rj[3 + ax], sg * Rj[6 + ax]};
                        REAL r[3] = {world[i].t[0] - world[j].t[0], world[i].t[1] - world[j].t[1], world[i].t[2] - world[j].t[2]};
                        dp[0] = w[1] * r[2] - w[2] * r[1]; dp[1] = w[2] * r[0] - w[0] * r[2]; dp[2] = w[0] * r[1] - w[1] * r[0];
                        const REAL* Ri = world[i].R;
                        for (int c = 0; c < 3; ++c) {                 /* dR = [w]x R_i, column by column */
                            REAL v[3] = {Ri[c], Ri[3 + c], Ri[6 + c]};
                            dR[c] = w[1] * v[2] - w[2] * v[1]; dR[3 + c] = w[2] * v[0] - w[0] * v[2]; dR[6 + c] = w[0] * v[1] - w[1] * v[0];
                        }
                    }
                }
                REAL dq[4];
                FN(quat_jvp)(world[i].R, dR, dq);
                for (int k = 0; k < 3; ++k) Js[(i * 7 + k) * D + d] = dp[k];
                for (int k = 0; k < 4; ++k) Js[(i * 7 + 3 + k) * D + d] = dq[k];
            }
        }
    }
}

/* quaternion.py:135-166 rotation_matrix_to_q: four candidates, pick the one with the largest
 * denominator (argmax of q_abs), denominators floored at 0.1.  R: packed 3x3, -> wxyz. */
void FN(orc_rotmat_to_quat)(const REAL* R, int64_t n, REAL* out) {
    for (int64_t s = 0; s < n; ++s) {
        const REAL* m = R + 9 * s;
        REAL m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
        REAL a[4] = {1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22};
        REAL qa[4];
        for (int k = 0; k < 4; ++k) qa[k] = a[k] > 0 ? SQRT(a[k]) : 0;      /* sqrt_with_mask */
        REAL cand[4][4] = {
            {qa[0] * qa[0], m21 - m12, m02 - m20, m10 - m01},
            {m21 - m12, qa[1] * qa[1], m10 + m01, m02 + m20},
            {m02 - m20, m10 + m01, qa[2] * qa[2], m12 + m21},
            {m10 - m01, m20 + m02, m21 + m12, qa[3] * qa[3]}};
        int best = 0;
        for (int k = 1; k < 4; ++k) if (qa[k] > qa[best]) best = k;          /* argmax: first max */
        REAL den = 2 * (qa[best] > (REAL)0.1 ? qa[best] : (REAL)0.1);
        for (int k = 0; k < 4; ++k) out[4 * s + k] = cand[best][k] / den;
    }
}

/* spatial_vector.py:8-47 x_rot / y_rot / z_rot (kind 0 / 1 / 2) and quaternion.py:102-120 q_to_rotation_matrix (kind 3, wxyz) */
void FN(orc_rotation_from)(int kind, const REAL* in, int64_t n, REAL* R) {
    for (int64_t s = 0; s < n; ++s) {
        REAL* r = R + 9 * s;
        for (int k = 0; k < 9; ++k) r[k] = 0;
        if (kind == 3) {
            REAL w = in[4 * s], x = in[4 * s + 1], y = in[4 * s + 2], z = in[4 * s + 3];
            REAL dc = (REAL)2 / (((w * w + x * x) + y * y) + z * z);
            r[0] = 1 - dc * (y * y + z * z); r[1] = dc * (x * y - z * w); r[2] = dc * (x * z + y * w);
            r[3] = dc * (x * y + z * w); r[4] = 1 - dc * (x * x + z * z); r[5] = dc * (y * z - x * w);
            r[6] = dc * (x * z - y * w); r[7] = dc * (y * z + x * w); r[8] = 1 - dc * (x * x + y * y);
        } else {
            REAL c = COS(in[s]), sn = SIN(in[s]);
            if (kind == 0) { r[0] = 1; r[4] = c; r[5] = -sn; r[7] = sn; r[8] = c; }
            else if (kind == 1) { r[0] = c; r[2] = sn; r[4] = 1; r[6] = -sn; r[8] = c; }
            else { r[0] = c; r[1] = -sn; r[3] = sn; r[4] = c; r[8] = 1; }
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * Frame algebra (geometrics/frame.py:55-121) on packed poses R [n,9], t [n,3]; a frame with n == 1 broadcasts.
 * ------------------------------------------------------------------------------------------ */
/* frame.py:57-62 inverse: (R^T, -(R^T t)) */
static void FN(frm_inverse)(const REAL* R, const REAL* t, REAL* Ro, REAL* to) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Ro[3 * i + j] = R[3 * j + i];
        to[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
    }
}
/* geometrics/utils.py:11-17 multiply_transform: (Ra Rb, Ra tb + ta) */
static void FN(frm_compose2)(const REAL* Ra, const REAL* ta, const REAL* Rb, const REAL* tb, REAL* Ro, REAL* to) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Ro[3 * i + j] = Ra[3 * i] * Rb[j] + Ra[3 * i + 1] * Rb[3 + j] + Ra[3 * i + 2] * Rb[6 + j];
        to[i] = (Ra[3 * i] * tb[0] + Ra[3 * i + 1] * tb[1] + Ra[3 * i + 2] * tb[2]) + ta[i];
    }
}
/* op: TRK_FRAME_COMPOSE a o b (frame.py:64-68) | TRK_FRAME_INVERSE a^-1 | TRK_FRAME_INV_COMPOSE b^-1 o a (frame.py:70-76,
 * geometrics/utils.py:21-29) */
void FN(orc_frame_compose)(int op, const REAL* Ra, const REAL* ta, int64_t na, const REAL* Rb, const REAL* tb, int64_t nb,
                           REAL* Ro, REAL* to) {
    int64_t n = op == TRK_FRAME_INVERSE ? na : (na > nb ? na : nb);
    for (int64_t s = 0; s < n; ++s) {
        const REAL *ra = Ra + 9 * (na == 1 ? 0 : s), *va = ta + 3 * (na == 1 ? 0 : s);
        if (op == TRK_FRAME_INVERSE) { FN(frm_inverse)(ra, va, Ro + 9 * s, to + 3 * s); continue; }
        const REAL *rb = Rb + 9 * (nb == 1 ? 0 : s), *vb = tb + 3 * (nb == 1 ? 0 : s);
        if (op == TRK_FRAME_COMPOSE) FN(frm_compose2)(ra, va, rb, vb, Ro + 9 * s, to + 3 * s);
        else {
            REAL ri[9], ti[3];
            FN(frm_inverse)(rb, vb, ri, ti);
            FN(frm_compose2)(ri, ti, ra, va, Ro + 9 * s, to + 3 * s);
        }
    }
}
/* reverse mode of the three ops by the chain rule on the two primitives above (what autograd does with the reference's
 * matmuls): equal batch sizes */
static void FN(frm_mul_bwd)(const REAL* Ra, const REAL* Rb, const REAL* tb, const REAL* gR, const REAL* gt, REAL* gRa,
                             REAL* gta, REAL* gRb, REAL* gtb) {
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) {
            gRa[3 * i + k] = gR[3 * i] * Rb[3 * k] + gR[3 * i + 1] * Rb[3 * k + 1] + gR[3 * i + 2] * Rb[3 * k + 2] + gt[i] * tb[k];
            gRb[3 * i + k] = Ra[i] * gR[k] + Ra[3 + i] * gR[3 + k] + Ra[6 + i] * gR[6 + k];
        }
        gta[i] = gt[i];
        gtb[i] = Ra[i] * gt[0] + Ra[3 + i] * gt[1] + Ra[6 + i] * gt[2];
    }
}
static void FN(frm_inverse_bwd)(const REAL* R, const REAL* t, const REAL* gR, const REAL* gt, REAL* gRa, REAL* gta) {
    for (int j = 0; j < 3; ++j) {
        for (int i = 0; i < 3; ++i) gRa[3 * j + i] = gR[3 * i + j] - t[j] * gt[i];
        gta[j] = -(R[3 * j] * gt[0] + R[3 * j + 1] * gt[1] + R[3 * j + 2] * gt[2]);
    }
}
void FN(orc_frame_compose_backward)(int op, const REAL* Ra, const REAL* ta, const REAL* Rb, const REAL* tb, const REAL* gR,
                                    const REAL* gt, int64_t n, REAL* gRa, REAL* gta, REAL* gRb, REAL* gtb) {
    for (int64_t s = 0; s < n; ++s) {
        const REAL *ra = Ra + 9 * s, *va = ta + 3 * s, *g9 = gR + 9 * s, *g3 = gt + 3 * s;
        if (op == TRK_FRAME_INVERSE) { FN(frm_inverse_bwd)(ra, va, g9, g3, gRa + 9 * s, gta + 3 * s); continue; }
        const REAL *rb = Rb + 9 * s, *vb = tb + 3 * s;
        if (op == TRK_FRAME_COMPOSE) FN(frm_mul_bwd)(ra, rb, vb, g9, g3, gRa + 9 * s, gta + 3 * s, gRb + 9 * s, gtb + 3 * s);
        else {
            REAL ri[9], ti[3], gri[9], gti[3];
            FN(frm_inverse)(rb, vb, ri, ti);
            FN(frm_mul_bwd)(ri, ra, va, g9, g3, gri, gti, gRa + 9 * s, gta + 3 * s);
            FN(frm_inverse_bwd)(rb, vb, gri, gti, gRb + 9 * s, gtb + 3 * s);
        }
    }
}
/* frame.py:116-118 transform_point: out[s,p,:] = R_s point_p + t_s; reverse mode w.r.t. the pose when g != NULL */
void FN(orc_frame_transform_points)(const REAL* R, const REAL* t, int64_t n, const REAL* pts, int P, REAL* out, const REAL* g,
                                    REAL* gR, REAL* gt) {
    for (int64_t s = 0; s < n; ++s) {
        const REAL* r = R + 9 * s;
        for (int p = 0; p < P; ++p)
            for (int i = 0; i < 3; ++i)
                out[(s * P + p) * 3 + i] = (r[3 * i] * pts[3 * p] + r[3 * i + 1] * pts[3 * p + 1] + r[3 * i + 2] * pts[3 * p + 2]) + t[3 * s + i];
        if (!g) continue;
        for (int k = 0; k < 9; ++k) gR[9 * s + k] = 0;
        for (int k = 0; k < 3; ++k) gt[3 * s + k] = 0;
        for (int p = 0; p < P; ++p)
            for (int i = 0; i < 3; ++i) {
                REAL gi = g[(s * P + p) * 3 + i];
                for (int k = 0; k < 3; ++k) gR[9 * s + 3 * i + k] += gi * pts[3 * p + k];
                gt[3 * s + i] += gi;
            }
    }
}
/* frame.py:87-114 get_quaternion (XYZW) and frame.py:120-121 get_euler */
void FN(orc_frame_quat_euler)(const REAL* R, int64_t n, REAL* quat_xyzw, REAL* euler) {
    for (int64_t s = 0; s < n; ++s) {
        REAL w[4];
        FN(frame_quat_wxyz)(R + 9 * s, w);
        quat_xyzw[4 * s] = w[1]; quat_xyzw[4 * s + 1] = w[2]; quat_xyzw[4 * s + 2] = w[3]; quat_xyzw[4 * s + 3] = w[0];
        const REAL* r = R + 9 * s;
        euler[3 * s] = ATAN2(r[7], r[8]); euler[3 * s + 1] = ASIN(-r[6]); euler[3 * s + 2] = ATAN2(r[3], r[0]);
    }
}

/* ------------------------------------------------------------------------------------------
 * Signed distance fields
 * ------------------------------------------------------------------------------------------ */
/* One primitive at object-frame point x: value and gradient w.r.t. x.
 * sphere      primitives.py:108-112   ||x-c|| - r                  (torch.norm backward: 0 at x == c)
 * rounded box primitives.py:327-334   min(max_k u,0) + ||relu(u)|| - r,  u = |x-c| - half + r
 * sharp box   primitives.py:220-223   max_k(|x-c| - half)                                         */
static inline REAL FN(prim_sdf)(const TrkPrimitive* p, const REAL* x, REAL* g) {
    REAL d[3] = {x[0] - (REAL)p->center[0], x[1] - (REAL)p->center[1], x[2] - (REAL)p->center[2]};
    if (p->type == TRK_PRIM_SPHERE) {
        REAL nrm = SQRT(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        for (int k = 0; k < 3; ++k) g[k] = nrm > 0 ? d[k] / nrm : 0;
        return nrm - (REAL)p->radius;
    }
    REAL sg[3], u[3];
    for (int k = 0; k < 3; ++k) { sg[k] = d[k] > 0 ? 1 : (d[k] < 0 ? -1 : 0); }
    if (p->type == TRK_PRIM_SHARP_BOX) {
        int am = 0;
        for (int k = 0; k < 3; ++k) u[k] = FABS(d[k]) - (REAL)p->half[k];
        for (int k = 1; k < 3; ++k) if (u[k] > u[am]) am = k;
        for (int k = 0; k < 3; ++k) g[k] = (k == am) ? sg[k] : 0;
        return u[am];
    }
    REAL r = (REAL)p->radius;
    for (int k = 0; k < 3; ++k) u[k] = FABS(d[k]) - (REAL)p->half[k] + r;
    int am = 0;
    for (int k = 1; k < 3; ++k) if (u[k] > u[am]) am = k;
    REAL maxu = u[am];
    REAL ru[3], nn = 0;
    for (int k = 0; k < 3; ++k) { ru[k] = u[k] > 0 ? u[k] : 0; nn += ru[k] * ru[k]; }
    nn = SQRT(nn);
    for (int k = 0; k < 3; ++k) {
        REAL gk = nn > 0 ? ru[k] / nn : 0;
        if (maxu < 0 && k == am) gk += 1;
        g[k] = gk * sg[k];
    }
    return (maxu < 0 ? maxu : 0) + nn - r;
}

/* grid_map_sdf.py:84-114 get_sdf: nearest-lower cell, stored gradient */
static inline REAL FN(grid_sdf)(const TrkGridDesc* gd, const REAL* x, REAL* g) {
    int idx[3];
    for (int k = 0; k < 3; ++k) {
        REAL f = FLOOR((x[k] - (REAL)gd->lim_min[k]) / (REAL)gd->map_dim[k] * (REAL)gd->dims[k]);
        int v = (int)f;
        if (v < 0) v = 0;
        if (v > gd->dims[k] - 1) v = gd->dims[k] - 1;
        idx[k] = v;
    }
    int64_t lin = ((int64_t)idx[0] * gd->dims[1] + idx[1]) * gd->dims[2] + idx[2];
    for (int k = 0; k < 3; ++k) g[k] = (REAL)gd->grad[3 * lin + k];
    return (REAL)gd->sdf[lin];
}

/* primitives.py:387-405 ObjectField: x' = R^T (x - pos); min over the object's primitives;
 * gradient back through the rotation: g = R g' */
static inline REAL FN(object_sdf)(const TrkCostModelDesc* c, int o, const REAL* x, REAL* g) {
    const TrkObject* ob = &c->objects[o];
    if (ob->is_grid) return FN(grid_sdf)(&c->grid, x, g);
    REAL R[9], d[3], xl[3], best = 0, gb[3] = {0, 0, 0};
    for (int k = 0; k < 9; ++k) R[k] = (REAL)ob->R[k];
    for (int k = 0; k < 3; ++k) d[k] = x[k] - (REAL)ob->pos[k];
    FN(mat3T_vec)(R, d, xl);
    int first = 1;
    for (int pi = ob->prim_begin; pi < ob->prim_end; ++pi) {
        REAL gp[3];
        REAL v = FN(prim_sdf)(&c->prims[pi], xl, gp);
        if (first || v < best) { best = v; gb[0] = gp[0]; gb[1] = gp[1]; gb[2] = gp[2]; first = 0; }
    }
    FN(mat3_vec)(R, gb, g);
    return best;
}

/* distance_fields.py:107-124 compute_embodiment_cost (field_type='sdf') for the selected fields:
 *   objects  :298-316  sum_l max_o (margin_l - sdf_o(p_l))
 *   ws box   :319-332  six plane "objects": [p - ws_min ; ws_max - p]
 *   self     :194-208  sum_pairs (margin_ij - ||p_i - p_j||)
 * pos [n_links_in,3] one sample; gpos accumulates d cost / d pos (may be NULL). Returns the cost. */
static REAL FN(cost_fields_core)(const TrkCostModelDesc* c, int fields, const REAL* pos, REAL* gpos) {
    REAL cost = 0;
    if (fields & TRK_FIELD_OBJECTS) {
        for (int l = 0; l < c->n_obj_links; ++l) {
            int li = c->obj_link_idx[l];
            REAL best = 0, gb[3] = {0, 0, 0};
            for (int o = 0; o < c->n_objects; ++o) {
                REAL g[3];
                REAL v = (REAL)c->obj_link_margin[l] - FN(object_sdf)(c, o, pos + 3 * li, g);
                if (o == 0 || v > best) { best = v; gb[0] = -g[0]; gb[1] = -g[1]; gb[2] = -g[2]; }
            }
            if (c->n_objects > 0 && !((c->clamp_fields & TRK_FIELD_OBJECTS) && !(best > 0))) {   /* relu: value and gradient 0 at <= 0 */
                cost += best;
                if (gpos) for (int k = 0; k < 3; ++k) gpos[3 * li + k] += gb[k];
            }
        }
    }
    if ((fields & TRK_FIELD_WS) && c->has_ws) {
        for (int l = 0; l < c->n_obj_links; ++l) {
            int li = c->obj_link_idx[l];
            REAL best = 0; int bk = -1;
            for (int k = 0; k < 6; ++k) {
                REAL sd = k < 3 ? pos[3 * li + k] - (REAL)c->ws_min[k] : (REAL)c->ws_max[k - 3] - pos[3 * li + k - 3];
                REAL v = (REAL)c->obj_link_margin[l] - sd;
                if (bk < 0 || v > best) { best = v; bk = k; }
            }
            if ((c->clamp_fields & TRK_FIELD_WS) && !(best > 0)) continue;
            cost += best;
            if (gpos) gpos[3 * li + (bk % 3)] += bk < 3 ? (REAL)-1 : (REAL)1;
        }
    }
    if (fields & TRK_FIELD_SELF) {
        for (int pi = 0; pi < c->n_self_pairs; ++pi) {
            int a = c->self_link_idx[c->self_pairs[2 * pi]], b = c->self_link_idx[c->self_pairs[2 * pi + 1]];
            if (a == b) {   /* one self-collision link, distance_fields.py:195-198: torch.abs(link_pos).sum(-1) * 1e9 */
                REAL l1 = (FABS(pos[3 * a]) + FABS(pos[3 * a + 1])) + FABS(pos[3 * a + 2]);
                REAL v = (REAL)c->self_margin[pi] - l1 * (REAL)1e9;
                if ((c->clamp_fields & TRK_FIELD_SELF) && !(v > 0)) continue;
                cost += v;
                if (gpos) for (int k = 0; k < 3; ++k)       /* d|x|/dx = sign(x), 0 at 0 (torch.abs) */
                    gpos[3 * a + k] -= (REAL)1e9 * (pos[3 * a + k] > 0 ? (REAL)1 : (pos[3 * a + k] < 0 ? (REAL)-1 : (REAL)0));
                continue;
            }
            REAL d[3] = {pos[3 * a] - pos[3 * b], pos[3 * a + 1] - pos[3 * b + 1], pos[3 * a + 2] - pos[3 * b + 2]};
            REAL nrm = SQRT(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if ((c->clamp_fields & TRK_FIELD_SELF) && !((REAL)c->self_margin[pi] - nrm > 0)) continue;
            cost += (REAL)c->self_margin[pi] - nrm;
            if (gpos && nrm > 0)
                for (int k = 0; k < 3; ++k) { gpos[3 * a + k] -= d[k] / nrm; gpos[3 * b + k] += d[k] / nrm; }
        }
    }
    return cost;
}

/* interpolate_link_pos (interpolate_points_v1 distance_fields.py:66-69, applied at :145-147): the cost model's virtual columns
 * n_links_in + k = w0 * column src0 + w1 * column src1 (F.interpolate linear / align_corners=True unrolled on the host).
 * ext [(n_links_in + n_virtual) * 3] <- pos [n_links_in * 3] followed by the interpolated points. */
#define ORC_MAX_COLS (4 * TRK_MAX_LINKS + TRK_MAX_VIRTUAL)
static void FN(extend_columns)(const TrkCostModelDesc* c, const REAL* pos, REAL* ext) {
    int Lin = c->n_links_in;
    for (int k = 0; k < 3 * Lin; ++k) ext[k] = pos[k];
    for (int v = 0; v < c->n_virtual; ++v)
        for (int k = 0; k < 3; ++k)
            ext[3 * (Lin + v) + k] = (REAL)c->virtual_w[2 * v] * pos[3 * c->virtual_src[2 * v] + k] +
                                     (REAL)c->virtual_w[2 * v + 1] * pos[3 * c->virtual_src[2 * v + 1] + k];
}
/* one sample: pos [n_links_in, 3]; gpos (nullable) [n_links_in, 3] accumulates d cost / d pos, the adjoint of an interpolated
 * point going to its two source columns with its weights */
static REAL FN(cost_fields_sample)(const TrkCostModelDesc* c, int fields, const REAL* pos, REAL* gpos) {
    if (c->n_virtual == 0) return FN(cost_fields_core)(c, fields, pos, gpos);
    int Lin = c->n_links_in, W = Lin + c->n_virtual;
    REAL ext[ORC_MAX_COLS * 3], gext[ORC_MAX_COLS * 3];
    FN(extend_columns)(c, pos, ext);
    for (int k = 0; k < 3 * W; ++k) gext[k] = 0;
    REAL cost = FN(cost_fields_core)(c, fields, ext, gpos ? gext : NULL);
    if (gpos) {
        for (int k = 0; k < 3 * Lin; ++k) gpos[k] += gext[k];
        for (int v = 0; v < c->n_virtual; ++v)
            for (int k = 0; k < 3; ++k) {
                gpos[3 * c->virtual_src[2 * v] + k] += (REAL)c->virtual_w[2 * v] * gext[3 * (Lin + v) + k];
                gpos[3 * c->virtual_src[2 * v + 1] + k] += (REAL)c->virtual_w[2 * v + 1] * gext[3 * (Lin + v) + k];
            }
    }
    return cost;
}

void FN(orc_cost_fields)(const TrkCostModelDesc* c, int fields, const REAL* link_pos, int64_t n,
                         REAL* cost, REAL* g_link_pos) {
    int Lin = c->n_links_in;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        REAL* g = g_link_pos ? g_link_pos + s * Lin * 3 : NULL;
        if (g) for (int k = 0; k < 3 * Lin; ++k) g[k] = 0;
        cost[s] = FN(cost_fields_sample)(c, fields, link_pos + s * Lin * 3, g);
    }
}

/* distance_fields.py:210-215 (self: any d < margin) and :283-291 (objects/ws: any sdf < margin);
 * margin_override NaN = defaults (per-pair / per-link+cutoff). tasks.py:227-228 ORs the fields. */
void FN(orc_collision_fields)(const TrkCostModelDesc* c, int fields, const REAL* link_pos, int64_t n,
                              REAL margin_override, uint8_t* out) {
    int Lin = c->n_links_in;
    int use_default = margin_override != margin_override;
    for (int64_t s = 0; s < n; ++s) {
        REAL ext[ORC_MAX_COLS * 3];
        const REAL* pos = link_pos + s * Lin * 3;
        if (c->n_virtual > 0) { FN(extend_columns)(c, pos, ext); pos = ext; }
        int hit = 0;
        if (fields & TRK_FIELD_OBJECTS)
            for (int l = 0; l < c->n_obj_links; ++l)
                for (int o = 0; o < c->n_objects; ++o) {
                    REAL g[3];
                    REAL mg = use_default ? (REAL)c->obj_link_margin[l] : margin_override;
                    if (FN(object_sdf)(c, o, pos + 3 * c->obj_link_idx[l], g) < mg) hit = 1;
                }
        if ((fields & TRK_FIELD_WS) && c->has_ws)
            for (int l = 0; l < c->n_obj_links; ++l)
                for (int k = 0; k < 6; ++k) {
                    int li = c->obj_link_idx[l];
                    REAL sd = k < 3 ? pos[3 * li + k] - (REAL)c->ws_min[k] : (REAL)c->ws_max[k - 3] - pos[3 * li + k - 3];
                    REAL mg = use_default ? (REAL)c->obj_link_margin[l] : margin_override;
                    if (sd < mg) hit = 1;
                }
        if (fields & TRK_FIELD_SELF)
            for (int pi = 0; pi < c->n_self_pairs; ++pi) {
                int a = c->self_link_idx[c->self_pairs[2 * pi]], b = c->self_link_idx[c->self_pairs[2 * pi + 1]];
                REAL d[3] = {pos[3 * a] - pos[3 * b], pos[3 * a + 1] - pos[3 * b + 1], pos[3 * a + 2] - pos[3 * b + 2]};
                REAL mg = use_default ? (REAL)c->self_margin[pi] : margin_override;
                if (a == b) {       /* distance_fields.py:195-198 */
                    if (((FABS(pos[3 * a]) + FABS(pos[3 * a + 1])) + FABS(pos[3 * a + 2])) * (REAL)1e9 < mg) hit = 1;
                    continue;
                }
                if (SQRT(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < mg) hit = 1;
            }
        out[s] = (uint8_t)hit;
    }
}

/* distance_fields.py:347-356 + geometrics/utils.py:130-154,209-224:
 * d = w_rot*(1 - (tr(R Rt^T) - 1)/2) + w_pos*||p - pt||  (each term only if its weight > 0); cost = d^2 if square.
 * H, Ht: row-major 4x4.  gH (nullable, 16 floats) receives d cost / d H (3x4 block, rest zero). */
static REAL FN(ee_cost_sample)(const REAL* H, const REAL* Ht, REAL w_pos, REAL w_rot, int square, REAL* gH) {
    REAL tr = 0, d = 0, dp[3], nrm = 0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) tr += H[4 * r + c] * Ht[4 * r + c];
    if (w_rot > 0) d += w_rot * (1 - (tr - 1) * (REAL)0.5);
    for (int k = 0; k < 3; ++k) { dp[k] = H[4 * k + 3] - Ht[4 * k + 3]; nrm += dp[k] * dp[k]; }
    nrm = SQRT(nrm);
    if (w_pos > 0) d += w_pos * nrm;
    if (gH) {
        REAL sc = square ? 2 * d : 1;
        for (int k = 0; k < 16; ++k) gH[k] = 0;
        if (w_rot > 0) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) gH[4 * r + c] = sc * (-(REAL)0.5 * w_rot) * Ht[4 * r + c];
        if (w_pos > 0 && nrm > 0) for (int k = 0; k < 3; ++k) gH[4 * k + 3] = sc * w_pos * dp[k] / nrm;
    }
    return square ? d * d : d;
}

void FN(orc_ee_cost)(const TrkCostModelDesc* c, const REAL* H, int64_t n, const REAL* target, int per_sample,
                     REAL* cost, REAL* gH) {
    for (int64_t s = 0; s < n; ++s) {
        REAL Ht[16];
        for (int k = 0; k < 16; ++k) Ht[k] = target ? target[(per_sample ? s * 16 : 0) + k] : (REAL)c->ee_target[k];
        cost[s] = FN(ee_cost_sample)(H + s * 16, Ht, (REAL)c->ee_w_pos, (REAL)c->ee_w_rot, c->ee_square, gH ? gH + s * 16 : NULL);
    }
}

/* Fused rollout = tasks.py:206-230 (FK once, the three collision fields on link origins) + EE cost
 * + backward to q.  cost [n], gq [n,D], link_pos (nullable) [n,L,3]. */
void FN(orc_rollout)(const TrkKinModelDesc* m, const TrkCostModelDesc* c, const TrkRolloutWeights* w,
                     const REAL* q, int64_t n, REAL* link_pos, REAL* cost, REAL* gq) {
    int L = m->n_links, D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        REAL pos[TRK_MAX_LINKS * 3], gpos[TRK_MAX_LINKS * 3], gH[TRK_MAX_LINKS * 16], tmp[TRK_MAX_LINKS * 3];
        FN(fk_sample)(m, q + s * D, world, NULL, NULL);
        for (int i = 0; i < L; ++i) for (int k = 0; k < 3; ++k) pos[3 * i + k] = world[i].t[k];
        if (link_pos) for (int k = 0; k < 3 * L; ++k) link_pos[s * L * 3 + k] = pos[k];
        for (int k = 0; k < 3 * L; ++k) gpos[k] = 0;
        for (int k = 0; k < 16 * L; ++k) gH[k] = 0;
        REAL total = 0;
        const REAL ws[3] = {(REAL)w->w_self, (REAL)w->w_obj, (REAL)w->w_ws};
        const int fl[3] = {TRK_FIELD_SELF, TRK_FIELD_OBJECTS, TRK_FIELD_WS};
        for (int f = 0; f < 3; ++f) {
            if (ws[f] == 0) continue;
            for (int k = 0; k < 3 * L; ++k) tmp[k] = 0;
            total += ws[f] * FN(cost_fields_sample)(c, fl[f], pos, tmp);
            for (int k = 0; k < 3 * L; ++k) gpos[k] += ws[f] * tmp[k];
        }
        for (int i = 0; i < L; ++i) for (int k = 0; k < 3; ++k) gH[16 * i + 4 * k + 3] = gpos[3 * i + k];
        if (w->w_ee != 0 && c->ee_link >= 0) {
            /* one EESE3DistanceField per tracked link (the second one: two-arm scenes), same weights */
            const int links[2] = {c->ee_link, c->ee2_link};
            const float* targets[2] = {c->ee_target, c->ee2_target};
            for (int e = 0; e < 2; ++e) {
                if (links[e] < 0) continue;
                REAL H[16], Ht[16], g[16];
                FN(pose_to_H)(&world[links[e]], H);
                for (int k = 0; k < 16; ++k) Ht[k] = (REAL)targets[e][k];
                total += (REAL)w->w_ee * FN(ee_cost_sample)(H, Ht, (REAL)c->ee_w_pos, (REAL)c->ee_w_rot, c->ee_square, g);
                for (int k = 0; k < 12; ++k) gH[16 * links[e] + k] += (REAL)w->w_ee * g[k];
            }
        }
        cost[s] = total;
        FN(fk_backward_sample)(m, q + s * D, gH, gq + s * D);
    }
}

/* Points fixed in link frames: world = R_link off + t_link  (Frame.transform_point frame.py:116-118, as used for the
 * grasped-object collision points in RobotPanda.fk_map_collision_impl robot_panda.py:154-168). */
#ifndef ORC_MAX_POINTS
#define ORC_MAX_POINTS 192
#endif
static void FN(points_sample)(const FN(Pose)* world, const int32_t* plink, const float* poff, int P, REAL* out) {
    for (int k = 0; k < P; ++k) {
        const FN(Pose)* w = &world[plink[k]];
        for (int r = 0; r < 3; ++r) {
            REAL acc = 0;
            for (int c = 0; c < 3; ++c) acc += w->R[3 * r + c] * (REAL)poff[3 * k + c];
            out[3 * k + r] = acc + w->t[r];
        }
    }
}
/* adjoint of points_sample scattered into a link-pose adjoint gH [L,4,4]: tbar += g, Rbar += g off^T */
static void FN(points_adjoint)(const int32_t* plink, const float* poff, int P, const REAL* gpos, REAL* gH) {
    for (int k = 0; k < P; ++k) {
        REAL* g = gH + 16 * plink[k];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) g[4 * r + c] += gpos[3 * k + r] * (REAL)poff[3 * k + c];
            g[4 * r + 3] += gpos[3 * k + r];
        }
    }
}

void FN(orc_fk_points)(const TrkKinModelDesc* m, const int32_t* plink, const float* poff, int P, const REAL* q, int64_t n,
                       REAL* out) {
    int D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        FN(fk_sample)(m, q + s * D, world, NULL, NULL);
        FN(points_sample)(world, plink, poff, P, out + s * P * 3);
    }
}

void FN(orc_fk_points_backward)(const TrkKinModelDesc* m, const int32_t* plink, const float* poff, int P, const REAL* q,
                                const REAL* gpos, int64_t n, REAL* gq) {
    int L = m->n_links, D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        REAL gH[TRK_MAX_LINKS * 16];
        for (int k = 0; k < 16 * L; ++k) gH[k] = 0;
        FN(points_adjoint)(plink, poff, P, gpos + s * P * 3, gH);
        FN(fk_backward_sample)(m, q + s * D, gH, gq + s * D);
    }
}

/* orc_rollout with the collision fields evaluated on attached points (the cost model's columns index the points;
 * ee_link stays a link index). */
void FN(orc_rollout_points)(const TrkKinModelDesc* m, const int32_t* plink, const float* poff, int P,
                            const TrkCostModelDesc* c, const TrkRolloutWeights* w, const REAL* q, int64_t n,
                            REAL* point_pos, REAL* cost, REAL* gq) {
    int L = m->n_links, D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        REAL pos[ORC_MAX_POINTS * 3], gpos[ORC_MAX_POINTS * 3], tmp[ORC_MAX_POINTS * 3], gH[TRK_MAX_LINKS * 16];
        FN(fk_sample)(m, q + s * D, world, NULL, NULL);
        FN(points_sample)(world, plink, poff, P, pos);
        if (point_pos) for (int k = 0; k < 3 * P; ++k) point_pos[s * P * 3 + k] = pos[k];
        for (int k = 0; k < 3 * P; ++k) gpos[k] = 0;
        for (int k = 0; k < 16 * L; ++k) gH[k] = 0;
        REAL total = 0;
        const REAL ws[3] = {(REAL)w->w_self, (REAL)w->w_obj, (REAL)w->w_ws};
        const int fl[3] = {TRK_FIELD_SELF, TRK_FIELD_OBJECTS, TRK_FIELD_WS};
        for (int f = 0; f < 3; ++f) {
            if (ws[f] == 0) continue;
            for (int k = 0; k < 3 * P; ++k) tmp[k] = 0;
            total += ws[f] * FN(cost_fields_sample)(c, fl[f], pos, tmp);
            for (int k = 0; k < 3 * P; ++k) gpos[k] += ws[f] * tmp[k];
        }
        FN(points_adjoint)(plink, poff, P, gpos, gH);
        if (w->w_ee != 0 && c->ee_link >= 0) {
            /* one EESE3DistanceField per tracked link (the second one: two-arm scenes), same weights */
            const int links[2] = {c->ee_link, c->ee2_link};
            const float* targets[2] = {c->ee_target, c->ee2_target};
            for (int e = 0; e < 2; ++e) {
                if (links[e] < 0) continue;
                REAL H[16], Ht[16], g[16];
                FN(pose_to_H)(&world[links[e]], H);
                for (int k = 0; k < 16; ++k) Ht[k] = (REAL)targets[e][k];
                total += (REAL)w->w_ee * FN(ee_cost_sample)(H, Ht, (REAL)c->ee_w_pos, (REAL)c->ee_w_rot, c->ee_square, g);
                for (int k = 0; k < 12; ++k) gH[16 * links[e] + k] += (REAL)w->w_ee * g[k];
            }
        }
        cost[s] = total;
        FN(fk_backward_sample)(m, q + s * D, gH, gq + s * D);
    }
}

/* One iteration of DifferentiableTree.inverse_kinematics (robot_tree.py:345-377):
 *   valid  = all(lower <= q <= upper) and SE3_distance(FK(q)[link], H_target) < se3_eps      (ik_termination :419-442)
 *   loss   = SE3_distance(w_pos = w_rot = 1, not squared) + w_jl * sum hinge^2                (loss_fn_ik_per_q :386-417)
 *   q     <- Adam(q, d loss / d q)    (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8, no weight decay)
 * `valid` and `loss` refer to q BEFORE the update, as in the reference loop.  step = 1-based iteration count. */
void FN(orc_ik_step)(const TrkKinModelDesc* m, int link, const REAL* H_target, int per_sample, const REAL* lower,
                     const REAL* upper, REAL w_jl, REAL se3_eps, REAL lr, int step, int64_t n, REAL* q, REAL* mom,
                     REAL* vel, REAL* loss, REAL* grad, uint8_t* valid) {
    int L = m->n_links, D = m->n_dofs;
    const REAL b1 = (REAL)0.9, b2 = (REAL)0.999, eps = (REAL)1e-8;
    const REAL bc1 = 1 - POW(b1, (REAL)step), bc2 = 1 - POW(b2, (REAL)step);
    for (int64_t s = 0; s < n; ++s) {
        FN(Pose) world[TRK_MAX_LINKS];
        REAL gH[TRK_MAX_LINKS * 16], H[16], g[16], gq[TRK_MAX_DOFS];
        REAL* qs = q + s * D;
        FN(fk_sample)(m, qs, world, NULL, NULL);
        FN(pose_to_H)(&world[link], H);
        const REAL* Ht = H_target + (per_sample ? s * 16 : 0);
        REAL err = FN(ee_cost_sample)(H, Ht, 1, 1, 0, g);
        for (int k = 0; k < 16 * L; ++k) gH[k] = 0;
        for (int k = 0; k < 12; ++k) gH[16 * link + k] = g[k];
        FN(fk_backward_sample)(m, qs, gH, gq);
        int ok = err < se3_eps;
        REAL jl = 0;
        for (int d = 0; d < D; ++d) {
            if (qs[d] < lower[d]) { jl += (lower[d] - qs[d]) * (lower[d] - qs[d]); gq[d] += w_jl * -2 * (lower[d] - qs[d]); }
            if (qs[d] > upper[d]) { jl += (upper[d] - qs[d]) * (upper[d] - qs[d]); gq[d] += w_jl * -2 * (upper[d] - qs[d]); }
            if (!(qs[d] >= lower[d] && qs[d] <= upper[d])) ok = 0;
        }
        if (loss) loss[s] = err + w_jl * jl;
        if (valid) valid[s] = (uint8_t)ok;
        for (int d = 0; d < D; ++d) {
            if (grad) grad[s * D + d] = gq[d];
            if (lr > 0) {
                REAL* mm = mom + s * D + d; REAL* vv = vel + s * D + d;
                *mm = b1 * *mm + (1 - b1) * gq[d];
                *vv = b2 * *vv + (1 - b2) * gq[d] * gq[d];
                const REAL denom = SQRT(*vv) / SQRT(bc2) + eps;
                qs[d] -= (lr / bc1) * (*mm / denom);
            }
        }
    }
}

/* grid_map_sdf.py:34-63 precompute_sdf: linspace voxel centres (endpoints inclusive), value = min over
 * objects (compute_signed_distance_raw :65-73), gradient of that min. */
void FN(orc_grid_precompute)(const TrkCostModelDesc* c, const int32_t* dims, const REAL* lim_min, const REAL* lim_max,
                             REAL* sdf, REAL* grad) {
    for (int ix = 0; ix < dims[0]; ++ix)
        for (int iy = 0; iy < dims[1]; ++iy)
            for (int iz = 0; iz < dims[2]; ++iz) {
                int id[3] = {ix, iy, iz};
                REAL x[3];
                for (int k = 0; k < 3; ++k) {
                    /* torch.linspace(start, end, steps): start + i*step for the first half, end - (steps-1-i)*step after;
                     * a single node is the START, torch.linspace(lo, hi, 1) = [lo] */
                    REAL step = dims[k] > 1 ? (lim_max[k] - lim_min[k]) / (REAL)(dims[k] - 1) : 0;
                    x[k] = (dims[k] == 1 || id[k] < dims[k] / 2) ? lim_min[k] + step * id[k] : lim_max[k] - step * (dims[k] - 1 - id[k]);
                }
                REAL best = 0, gb[3] = {0, 0, 0};
                int first = 1;
                for (int o = 0; o < c->n_objects; ++o) {
                    if (c->objects[o].is_grid) continue;
                    REAL g[3];
                    REAL v = FN(object_sdf)(c, o, x, g);
                    if (first || v < best) { best = v; gb[0] = g[0]; gb[1] = g[1]; gb[2] = g[2]; first = 0; }
                }
                int64_t lin = ((int64_t)ix * dims[1] + iy) * dims[2] + iz;
                sdf[lin] = best;
                for (int k = 0; k < 3; ++k) grad[3 * lin + k] = gb[k];
            }
}

/* ObjectField.compute_signed_distance on arbitrary points: sdf [n, n_objects], grad [n, n_objects, 3] */
void FN(orc_sdf_points)(const TrkCostModelDesc* c, const REAL* pts, int64_t n, REAL* sdf, REAL* grad) {
    for (int64_t s = 0; s < n; ++s)
        for (int o = 0; o < c->n_objects; ++o) {
            REAL g[3];
            sdf[s * c->n_objects + o] = FN(object_sdf)(c, o, pts + 3 * s, g);
            if (grad) for (int k = 0; k < 3; ++k) grad[(s * c->n_objects + o) * 3 + k] = g[k];
        }
}


/* Constant-velocity GP prior (BUILD-DEFINED, see include/trk.h trk_gp_prior_cost_grad; no reference counterpart):
 * per DOF e_t = (p_t + dt v_t - p_{t+1}, v_t - v_{t+1}), Q^-1 = sigma^-2 [[12/dt^3, -6/dt^2], [-6/dt^2, 4/dt]],
 * cost[b] = w/2 sum e^T Q^-1 e;  gradients by the chain rule on the two factors each state takes part in. */
void FN(orc_gp_prior)(const REAL* q, const REAL* qd, int64_t B, int H, int D, REAL dt, REAL sigma, REAL w,
                      REAL* cost, REAL* gq, REAL* gqd) {
    const REAL s2 = 1 / (sigma * sigma);
    const REAL a = 12 * s2 / (dt * dt * dt), b = -6 * s2 / (dt * dt), c = 4 * s2 / dt;
#pragma omp parallel for schedule(static)
    for (int64_t tr = 0; tr < B; ++tr) {
        const REAL* p = q + tr * H * D; const REAL* v = qd + tr * H * D;
        REAL* gp = gq + tr * H * D; REAL* gv = gqd + tr * H * D;
        for (int k = 0; k < H * D; ++k) { gp[k] = 0; gv[k] = 0; }
        REAL acc = 0;
        for (int t = 0; t + 1 < H; ++t)
            for (int d = 0; d < D; ++d) {
                const int i = t * D + d, j = i + D;
                const REAL ep = p[i] + dt * v[i] - p[j], ev = v[i] - v[j];
                const REAL rp = a * ep + b * ev, rv = b * ep + c * ev;
                acc += (REAL)0.5 * (ep * rp + ev * rv);
                gp[i] += w * rp; gv[i] += w * (dt * rp + rv);
                gp[j] -= w * rp; gv[j] -= w * rv;
            }
        cost[tr] = w * acc;
    }
}


/* The same prior, factor by factor: out[b, t] = w/2 e_t^T Q^-1 e_t for the factor between t and t + 1 (0 at t = H - 1) -- how
 * trk_rollout_gp_cost_grad attributes the prior's cost to the samples (sum_t out[b, t] = orc_gp_prior's cost[b]). */
void FN(orc_gp_factor_cost)(const REAL* q, const REAL* qd, int64_t B, int H, int D, REAL dt, REAL sigma, REAL w, REAL* out) {
    const REAL s2 = 1 / (sigma * sigma);
    const REAL a = 12 * s2 / (dt * dt * dt), b = -6 * s2 / (dt * dt), c = 4 * s2 / dt;
    for (int64_t tr = 0; tr < B; ++tr) {
        const REAL* p = q + tr * H * D; const REAL* v = qd + tr * H * D;
        for (int t = 0; t < H; ++t) {
            REAL acc = 0;
            if (t + 1 < H)
                for (int d = 0; d < D; ++d) {
                    const int i = t * D + d, j = i + D;
                    const REAL ep = p[i] + dt * v[i] - p[j], ev = v[i] - v[j];
                    acc += (REAL)0.5 * (ep * (a * ep + b * ev) + ev * (b * ep + c * ev));
                }
            out[tr * H + t] = w * acc;
        }
    }
}

/* One damped Gauss-Newton (Levenberg-Marquardt) iteration of the batched IK -- BUILD-DEFINED (the reference's IK loop is Adam,
 * robot_tree.py:303-384; its geometric Jacobian :218-248 is what a Newton step is built from; parity unpinned, this restatement
 * is the definition the kernel trk_ik_gn_steps is checked against):
 *   (p, R, lin_jac, ang_jac) = orc_fk_jacobian(q) for `link`;   r = [p* - p ; rotvec(R* R^T)]  (world frame, the rotation vector
 *   from the quaternion (w, v) of R* R^T: v / |v| * 2 atan2(|v|, |w|), sign of v flipped when w < 0);
 *   lambda = damping + lm_gain |r|^2;   (J^T J + lambda I) dq = J^T r  by Cholesky;   q <- clamp(q + step_scale dq, lower, upper).
 * err [n] (nullable): SE3_distance (w_pos = w_rot = 1, geometrics/utils.py:130-154) of q AS PASSED IN -- the metric of the
 * reference's ik_termination (robot_tree.py:419-442). */
void FN(orc_ik_gn_step)(const TrkKinModelDesc* m, int link, const REAL* H_target, int per_sample, const REAL* lower, const REAL* upper,
                        REAL damping, REAL lm_gain, REAL step_scale, int64_t n, REAL* q, REAL* err) {
    const int D = m->n_dofs;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        REAL pos[3], quat[4], lin[3 * TRK_MAX_DOFS], ang[3 * TRK_MAX_DOFS];
        FN(orc_fk_jacobian)(m, q + s * D, NULL, 1, link, pos, quat, lin, ang, NULL, NULL);
        const REAL* Ht = H_target + (per_sample ? s * 16 : 0);
        /* current rotation from the quaternion the Jacobian routine returns would lose the matrix: walk again for R */
        FN(Pose) world[TRK_MAX_LINKS];
        {
            /* stateful walk (same quirks as orc_fk_jacobian): only the pose of `link` is needed */
            const int L = m->n_links;
            for (int p = 0; p < L; ++p) {
                int i = m->order[p];
                if (i == 0) { FN(base_pose)(m, &world[0]); continue; }
                FN(Pose) jp;
                int jt = m->joint_type[i];
                REAL qh = 0;
                if (jt != TRK_JOINT_FIXED) {
                    qh = q[s * D + m->dof_idx[i]];
                    if (m->sf_clamp[i]) { REAL lo = (REAL)m->lower[i], hi = (REAL)m->upper[i]; qh = qh < lo ? lo : (qh > hi ? hi : qh); }
                }
                for (int k = 0; k < 3; ++k) jp.t[k] = (REAL)m->trans[3 * i + k];
                REAL Rf[9];
                for (int k = 0; k < 9; ++k) Rf[k] = (REAL)m->R_fixed[9 * i + k];
                if (jt == TRK_JOINT_REVOLUTE || jt == TRK_JOINT_CONTINUOUS) {
                    REAL rot[9];
                    FN(axis_rot)(m->sf_rot_axis[i], qh, rot);
                    FN(mat3_mul)(Rf, rot, jp.R);
                } else {
                    for (int k = 0; k < 9; ++k) jp.R[k] = Rf[k];
                    if (jt == TRK_JOINT_PRISMATIC) for (int k = 0; k < 3; ++k) jp.t[k] += (REAL)m->axis[3 * i + k] * qh;
                }
                FN(pose_mul)(&world[m->parent[i]], &jp, &world[i]);
            }
        }
        const REAL* R = world[link].R;
        REAL r6[6], Re[9];
        for (int k = 0; k < 3; ++k) r6[k] = Ht[4 * k + 3] - pos[k];
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {            /* Re = R* R^T */
            REAL acc = 0;
            for (int k = 0; k < 3; ++k) acc += Ht[4 * a + k] * R[3 * b + k];
            Re[3 * a + b] = acc;
        }
        REAL qe[4];
        FN(frame_quat_wxyz)(Re, qe);
        REAL w = qe[0], v[3] = {qe[1], qe[2], qe[3]};
        if (w < 0) { w = -w; v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
        if (w > 1) w = 1;
        REAL nv = SQRT(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        REAL sc = 2 * ATAN2(nv, w) / (nv > (REAL)1e-12 ? nv : (REAL)1e-12);
        for (int k = 0; k < 3; ++k) r6[3 + k] = v[k] * sc;
        if (err) {
            REAL H[16] = {R[0], R[1], R[2], pos[0], R[3], R[4], R[5], pos[1], R[6], R[7], R[8], pos[2], 0, 0, 0, 1};
            err[s] = FN(ee_cost_sample)(H, Ht, 1, 1, 0, NULL);
        }
        REAL rr = 0;
        for (int k = 0; k < 6; ++k) rr += r6[k] * r6[k];
        const REAL lam = damping + lm_gain * rr;
        REAL A[TRK_MAX_DOFS][TRK_MAX_DOFS], g[TRK_MAX_DOFS];
        for (int i = 0; i < D; ++i) {
            REAL gi = 0;
            for (int k = 0; k < 3; ++k) gi += lin[k * D + i] * r6[k] + ang[k * D + i] * r6[3 + k];
            g[i] = gi;
            for (int j = 0; j <= i; ++j) {
                REAL a = 0;
                for (int k = 0; k < 3; ++k) a += lin[k * D + i] * lin[k * D + j] + ang[k * D + i] * ang[k * D + j];
                A[i][j] = a + (i == j ? lam : 0);
            }
        }
        /* Cholesky A = L L^T (lower triangle in place), then L y = g, L^T dq = y */
        for (int j = 0; j < D; ++j) {
            REAL d = A[j][j];
            for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
            d = SQRT(d > (REAL)1e-30 ? d : (REAL)1e-30);
            A[j][j] = d;
            for (int i = j + 1; i < D; ++i) {
                REAL a = A[i][j];
                for (int k = 0; k < j; ++k) a -= A[i][k] * A[j][k];
                A[i][j] = a / d;
            }
        }
        for (int i = 0; i < D; ++i) { REAL a = g[i]; for (int k = 0; k < i; ++k) a -= A[i][k] * g[k]; g[i] = a / A[i][i]; }
        for (int i = D - 1; i >= 0; --i) { REAL a = g[i]; for (int k = i + 1; k < D; ++k) a -= A[k][i] * g[k]; g[i] = a / A[i][i]; }
        for (int i = 0; i < D; ++i) {
            REAL qn = q[s * D + i] + step_scale * g[i];
            q[s * D + i] = qn < lower[i] ? lower[i] : (qn > upper[i] ? upper[i] : qn);
        }
    }
}


/* finite_difference_vector trajectory/utils.py:53-64 and sum_t ||x[t+1] - x[t]|| (metrics.py:7-12, 27-35) */
void FN(orc_finite_difference)(const REAL* x, int64_t B, int H, int D, REAL dt, int method, REAL* out) {
    for (int64_t b = 0; b < B; ++b)
        for (int t = 0; t < H; ++t)
            for (int d = 0; d < D; ++d) {
                const int64_t i = (b * H + t) * D + d;
                REAL v = 0;
                if (method == 0) { if (t + 1 < H) v = (x[i + D] - x[i]) / dt; }
                else if (method == 1) { if (t > 0) v = (x[i] - x[i - D]) / dt; }
                else { if (t > 0 && t + 1 < H) v = (x[i + D] - x[i - D]) / (2 * dt); }
                out[i] = v;
            }
}
void FN(orc_traj_diff_norm_sum)(const REAL* x, int64_t B, int H, int S, int c0, int D, REAL* out) {
    for (int64_t b = 0; b < B; ++b) {
        REAL acc = 0;
        for (int t = 0; t + 1 < H; ++t) {
            REAL n2 = 0;
            for (int d = 0; d < D; ++d) { REAL df = x[(b * H + t + 1) * S + c0 + d] - x[(b * H + t) * S + c0 + d]; n2 += df * df; }
            acc += SQRT(n2);
        }
        out[b] = acc;
    }
}

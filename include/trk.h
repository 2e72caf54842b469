/*
 * trk.h -- C ABI of libtrk.so: MI355X (gfx950) batched differentiable forward
 * kinematics + planning-objective kernels.
 *
 * This is the drop-in boundary for the hot path of anindex/torch_robotics
 * (SURVEY.md section 8b).  The reference has no FFI layer: its boundary is a set of
 * Python methods.  Each entry point below names the reference method whose
 * arithmetic it replaces (file:line relative to the reference repo); the Python
 * classes in torch_robotics_amd/ keep the reference's signatures and call these.
 *
 * Conventions
 *  - All tensor arguments are DEVICE pointers to contiguous row-major fp32 unless
 *    a comment says "host".  The caller allocates every input and output; the
 *    library owns only the opaque handles it returns.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Launches
 *    are asynchronous; the caller synchronises.  No hidden global state; handles
 *    are immutable except through the trk_*_set_* calls, which must not race with
 *    launches that use the handle.
 *  - Every function returns TRK_OK (0) or a negative TrkStatus and writes nothing
 *    on error.  Nothing throws or aborts across the boundary.
 *  - N = number of samples (batch x horizon folded, reference robot_panda.py:142),
 *    L = number of links (URDF file order), D = number of DOFs (file order of the
 *    non-fixed links, reference robot_tree.py:112-115).
 *  - Homogeneous transforms are 4x4 row-major with the translation in column 3 and
 *    bottom row [0,0,0,1] (reference frame.py:81-85).  Quaternions are wxyz.
 */
#ifndef TRK_H
#define TRK_H

#ifndef __HIPCC_RTC__       /* in-process device compilation of a generated unit: the integer types are built in */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define TRK_ABI_VERSION 5
#define TRK_MAX_LINKS 64
#define TRK_MAX_DOFS 32
#define TRK_MAX_POSE_SLOTS 8
#define TRK_MAX_OBJECTS 16
#define TRK_MAX_PRIMS 256
#define TRK_MAX_COLL_LINKS 192
#define TRK_MAX_SELF_PAIRS 1024
#define TRK_MAX_VIRTUAL 192

typedef enum TrkStatus {
    TRK_OK = 0,
    TRK_ERR_INVALID_ARG = -1,   /* null pointer, negative size, index out of range          */
    TRK_ERR_UNSUPPORTED = -2,   /* joint type / model size the kernels do not handle         */
    TRK_ERR_HIP = -3,           /* a HIP runtime call failed (see trk_last_error)            */
    TRK_ERR_NO_DEVICE = -4      /* no gfx950 device visible                                  */
} TrkStatus;

typedef enum TrkJointType {
    TRK_JOINT_FIXED = 0,
    TRK_JOINT_REVOLUTE = 1,
    TRK_JOINT_CONTINUOUS = 2,
    TRK_JOINT_PRISMATIC = 3,
    TRK_JOINT_UNSUPPORTED = 4
} TrkJointType;

typedef void* trk_stream_t;

/* ---------------------------------------------------------------------------------
 * Kinematic model.  Host arrays, copied once at create().  Produced by
 * torch_robotics_amd/kinmodel.py, which restates the reference's model build
 * (models/utils.py:199-313, rigid_body.py:74-123, robot_tree.py:77-126).
 * All per-link arrays are indexed by link (file order) unless marked "by position"
 * (= index into the DFS pre-order `order`).
 * --------------------------------------------------------------------------------- */
typedef struct TrkKinModelDesc {
    int32_t abi_version;        /* TRK_ABI_VERSION */
    int32_t n_links;            /* L <= TRK_MAX_LINKS */
    int32_t n_dofs;             /* D <= TRK_MAX_DOFS  */
    int32_t n_slots;            /* pose-stack slots used by parent_slot/store_slot */
    const int32_t* parent;      /* [L] parent link, -1 for the root (link 0) */
    const int32_t* joint_type;  /* [L] TrkJointType of the joint whose child is the link */
    const int32_t* dof_idx;     /* [L] DOF index or -1 */
    const float* R_fixed;       /* [L*9] Rz(yaw)Ry(pitch)Rx(roll), row-major (rigid_body.py:93) */
    const float* trans;         /* [L*3] joint origin xyz */
    const float* axis;          /* [L*3] raw <axis>, zeros when absent */
    const int32_t* rot_axis;    /* [L] stateless FK rotation axis 0/1/2 (rigid_body.py:163-168) */
    const float* rot_sign;      /* [L] sign(axis_k) in {-1,0,+1} */
    const int32_t* clamp;       /* [L] stateless FK clamps q to [lower,upper] (rigid_body.py:157-160) */
    const float* lower;         /* [L] */
    const float* upper;         /* [L] */
    const int32_t* sf_rot_axis; /* [L] stateful path axis, sign ignored (rigid_body.py:101-106,226-227) */
    const int32_t* sf_clamp;    /* [L] stateful path clamps whenever limits exist (rigid_body.py:218-224) */
    const int32_t* jac_axis;    /* [L] column of the world rotation used as joint axis (robot_tree.py:242-244) */
    const int32_t* joint_list_idx; /* [L] index of the link's joint in the URDF joint list (robot_tree.py:235-240) */
    const int32_t* order;       /* [L] DFS pre-order of links, order[0] == 0 */
    const int32_t* subtree_end; /* [L] by position: one past the last descendant's position */
    const int32_t* parent_slot; /* [L] by position: -1 = parent is the previous position, else slot to load */
    const int32_t* store_slot;  /* [L] by position: slot to keep this link's pose in, or -1 */
    float base_R[9];            /* root pose (robot_tree.py:133-134), identity by default */
    float base_t[3];
} TrkKinModelDesc;

typedef struct TrkModel TrkModel;

int trk_abi_version(void);
/* Human-readable text of the last error on the calling thread ("" if none). */
const char* trk_last_error(void);

int trk_model_create(const TrkKinModelDesc* desc, TrkModel** out);
void trk_model_destroy(TrkModel* model);
/* reference: DifferentiableTree.update_base_pose robot_tree.py:133-134 (pose already converted
 * to a rotation matrix on the host, quaternion.py:102-120).  Host pointers. */
int trk_model_set_base_pose(TrkModel* model, const float* R9, const float* t3);
int trk_model_n_links(const TrkModel* model);
int trk_model_n_dofs(const TrkModel* model);
/* 1 if a model-specialised (ahead-of-time unrolled) fused kernel exists for this model and is enabled. */
int trk_model_is_specialized(const TrkModel* model);
/* Switch between the model-specialised fused kernel (default when one was built for these tables) and the
 * table-driven one; both compute the same function (used by the parity tests to cover both). */
int trk_model_enable_specialized(TrkModel* model, int enable);
/* Number of model-specialised units registered with the library (ahead-of-time ones plus run-time compiled ones that were
 * dlopen'ed).  A unit compiled against another layout of the launch structures is refused at registration and not counted;
 * the run-time compiler (torch_robotics_amd/jit.py) uses this to detect -- and rebuild -- a stale on-disk unit. */
int trk_spec_count(void);

/* ---------------------------------------------------------------------------------
 * Forward kinematics (stateless path).
 * --------------------------------------------------------------------------------- */

/* reference: DifferentiableTree.compute_forward_kinematics_all_links robot_tree.py:267-301
 *            (+ DifferentiableRigidBody.forward_kinematics rigid_body.py:146-211,
 *               Frame.get_transform_matrix frame.py:81-85).
 * q [N,D] -> H_out [N, n_sel, 4, 4].  link_sel: host int32[n_sel] link indices in output
 * order (NULL = all L links in file order, n_sel ignored). */
int trk_fk_forward(const TrkModel* model, const float* q, int64_t n,
                   const int32_t* link_sel, int32_t n_sel, float* H_out, trk_stream_t stream);

/* Link origins only.  reference: RobotPanda.fk_map_collision_impl robot_panda.py:138-170
 * + link_pos_from_link_tensor geometrics/utils.py:321-328.
 * q [N,D] -> pos_out [N, n_sel, 3]. */
int trk_fk_positions(const TrkModel* model, const float* q, int64_t n,
                     const int32_t* link_sel, int32_t n_sel, float* pos_out, trk_stream_t stream);

/* Explicit reverse-mode of trk_fk_forward (replaces autograd through ~350 bmm nodes).
 * gH [N, n_sel, 4, 4] (bottom row ignored) -> gq [N,D]; zero where the reference clamps
 * (rigid_body.py:157-160). */
int trk_fk_backward(const TrkModel* model, const float* q, const float* gH, int64_t n,
                    const int32_t* link_sel, int32_t n_sel, float* gq, trk_stream_t stream);

/* Explicit reverse-mode of trk_fk_positions.  gpos [N, n_sel, 3] -> gq [N,D]. */
int trk_fk_positions_backward(const TrkModel* model, const float* q, const float* gpos, int64_t n,
                              const int32_t* link_sel, int32_t n_sel, float* gq, trk_stream_t stream);

/* ---- points rigidly attached to links ----------------------------------------------------------------------------
 * reference: RobotPanda.fk_map_collision_impl robot_panda.py:154-168 (grasped-object collision points,
 *            GraspedObjectPandaBox.get_base_points_for_collision objects.py:57-89) through Frame.transform_point
 *            frame.py:116-118:  world = R_link * offset + t_link.  A zero offset is the link origin, so a point set
 *            {all links, then the grasped points} is exactly what fk_map_collision returns: [N, L + G, 3].
 *            Also carries per-link collision spheres (data/configs/panda/panda_sphere_config.yaml).
 * point_link: host int32[n_points] link (file index) each point is fixed to; point_offset: host float[n_points*3]
 * in that link's frame.  Output column k is point k.  The handle owns small device tables; immutable afterwards. */
typedef struct TrkPointSet TrkPointSet;
#define TRK_MAX_POINTS 192
int trk_point_set_create(const TrkModel* model, const int32_t* point_link, const float* point_offset,
                         int32_t n_points, TrkPointSet** out);
void trk_point_set_destroy(TrkPointSet* ps);
int trk_point_set_size(const TrkPointSet* ps);
/* 1 if a generated fused kernel with exactly this point set baked in was built (see trk_model_is_specialized). */
int trk_point_set_is_specialized(const TrkPointSet* ps);

/* q [N,D] -> pos_out [N, n_points, 3]. */
int trk_fk_points(const TrkModel* model, const TrkPointSet* ps, const float* q, int64_t n, float* pos_out,
                  trk_stream_t stream);
/* Explicit reverse mode of trk_fk_points (replaces autograd through the FK recursion and transform_point):
 * gpos [N, n_points, 3] -> gq [N,D]; zero where the reference clamps (rigid_body.py:157-160). */
int trk_fk_points_backward(const TrkModel* model, const TrkPointSet* ps, const float* q, const float* gpos, int64_t n,
                           float* gq, trk_stream_t stream);

/* Stateful FK + geometric Jacobian of one link.
 * reference: DifferentiableTree.compute_forward_kinematics_and_geometric_jacobian
 *            robot_tree.py:218-248 (update_kinematic_state :136-190, Frame.get_quaternion
 *            frame.py:87-114, q_convert_wxyz quaternion.py:240-242).
 * q, qd [N,D] -> pos [N,3], quat_wxyz [N,4], lin_jac [N,3,D], ang_jac [N,3,D].
 * qd may be NULL (velocities are then not computed).  vel_lin / vel_ang [N,3] (the link's
 * spatial velocity in the link frame, spatial_vector.py:87-97) may be NULL. */
int trk_fk_jacobian(const TrkModel* model, const float* q, const float* qd, int64_t n, int32_t link,
                    float* pos, float* quat_wxyz, float* lin_jac, float* ang_jac,
                    float* vel_lin, float* vel_ang, trk_stream_t stream);

/* reference: DifferentiableTree.compute_analytical_jacobian_all_links robot_tree.py:250-265 (autograd Jacobian of
 * [pos(3), quat_wxyz(4)] of every link through the stateless FK and rotation_matrix_to_q).
 * q [N,D] -> J [N, L, 7, D]. */
int trk_fk_analytic_jacobian(const TrkModel* model, const float* q, int64_t n, float* J, trk_stream_t stream);

/* One iteration of the batched Adam IK, reference: DifferentiableTree.inverse_kinematics robot_tree.py:345-377 with
 * loss_fn_ik_per_q :386-417 (SE3_distance w_pos = w_rot = 1 + w_joint_limits * squared hinge on [lower, upper]) and
 * ik_termination :419-442.  In place: q [N,D] <- Adam(q, d loss / d q) with torch.optim.Adam's defaults (betas 0.9/0.999,
 * eps 1e-8), state adam_m / adam_v [N,D] (zero before step 1), step = 1-based iteration.  loss [N] and valid [N] (uint8:
 * inside the limits and SE3 error < se3_eps) are evaluated on q BEFORE the update, as in the reference loop; lr = 0 only
 * evaluates.  H_target: DEVICE [16] or [N,16]; lower / upper: DEVICE [D].  All nullable outputs may be NULL. */
int trk_ik_step(const TrkModel* model, int32_t link, const float* H_target, int32_t per_sample_target, const float* lower,
                const float* upper, float w_joint_limits, float se3_eps, float lr, int32_t step, int64_t n, float* q,
                float* adam_m, float* adam_v, float* loss, uint8_t* valid, trk_stream_t stream);

/* The same for n_steps consecutive iterations first_step, first_step + 1, ... in ONE launch per 32 iterations: the
 * configurations stay on the chip between iterations (the persistent form of the loop robot_tree.py:345-377).  Exactly
 * n_steps calls of trk_ik_step, except that loss / valid describe q as passed in (before the FIRST of the updates) -- a
 * caller that tests the termination condition every n_steps iterations loses nothing. */
int trk_ik_steps(const TrkModel* model, int32_t link, const float* H_target, int32_t per_sample_target, const float* lower,
                 const float* upper, float w_joint_limits, float se3_eps, float lr, int32_t first_step, int32_t n_steps,
                 int64_t n, float* q, float* adam_m, float* adam_v, float* loss, uint8_t* valid, trk_stream_t stream);

/* K damped Gauss-Newton (Levenberg-Marquardt) iterations of the batched IK in ONE launch -- BUILD-DEFINED: the reference's loop is
 * Adam (DifferentiableTree.inverse_kinematics robot_tree.py:303-384, served by trk_ik_steps); a Newton step is what its geometric
 * Jacobian (compute_forward_kinematics_and_geometric_jacobian robot_tree.py:218-248) is for.  Per sample and iteration:
 *   stateful FK + geometric Jacobian J (6 x D, the reference's column rule) of `link` at q;
 *   r = [p* - p ; rotation vector of R* R^T]  (world frame);   lambda = damping + lm_gain |r|^2;
 *   (J^T J + lambda I) dq = J^T r  (Cholesky);   q <- clamp(q + step_scale dq, lower, upper).
 * The Jacobian, the normal equations and their factor never leave the lane's registers (the two-launch form trk_fk_jacobian +
 * trk_jtj moves 416 bytes per sample and iteration).  H_target: DEVICE [16] (per_sample_target = 0) or [n,16]; lower / upper:
 * DEVICE [D]; q [n,D] in place; err [n] / valid [n] (nullable): SE3_distance(w_pos = w_rot = 1) of q AS PASSED IN and
 * `err < se3_eps and lower <= q <= upper` -- the metric and test of ik_termination (robot_tree.py:419-442), so that a caller
 * testing every K iterations sees what trk_ik_steps would report.  Checked against oracle/oracle_impl.inc: orc_ik_gn_step.
 * Served by generated kernels only (robots up to 9 DOF, the link a unit tracks): TRK_ERR_UNSUPPORTED otherwise. */
int trk_ik_gn_steps(const TrkModel* model, int32_t link, const float* H_target, int32_t per_sample_target, const float* lower,
                    const float* upper, float damping, float lm_gain, float step_scale, float se3_eps, int32_t n_steps, int64_t n,
                    float* q, float* err, uint8_t* valid, trk_stream_t stream);

/* reference: rotation_matrix_to_q quaternion.py:135-166 (via link_quat_from_link_tensor
 * geometrics/utils.py:341-344).  R: n matrices, `stride` floats apart, 3x3 block with row
 * pitch `row_pitch` (9/3 for packed rotations, 16/4 for 4x4 transforms).  -> quat_wxyz [n,4]. */
int trk_rotmat_to_quat(const float* R, int64_t n, int32_t stride, int32_t row_pitch,
                       float* quat_wxyz, trk_stream_t stream);

/* Rotation matrices from angles or quaternions: R [n,9] row-major.
 *   TRK_ROT_X / _Y / _Z   in = angle [n]      x_rot / y_rot / z_rot        geometrics/spatial_vector.py:8-47
 *   TRK_ROT_QUAT_WXYZ     in = quat  [n,4]    q_to_rotation_matrix         geometrics/quaternion.py:102-120
 * trk_rotation_from_backward: gR [n,9] -> gin, shaped like `in` ([n] angles, or [n,4] for the quaternion: the reference's
 * q_to_rotation_matrix is plain differentiable torch arithmetic, incl. the 2 / |q|^2 normalisation). */
#define TRK_ROT_X 0
#define TRK_ROT_Y 1
#define TRK_ROT_Z 2
#define TRK_ROT_QUAT_WXYZ 3
int trk_rotation_from(int32_t kind, const float* in, int64_t n, float* R_out, trk_stream_t stream);
int trk_rotation_from_backward(int32_t kind, const float* in, const float* gR, int64_t n, float* gin, trk_stream_t stream);

/* Frame algebra on packed poses: R [n,9] row-major, t [n,3] (reference: geometrics/frame.py:55-121, the `Frame`s that
 * compute_forward_kinematics_all_links(return_dict=True) returns, robot_tree.py:283-297).  A frame given once (na / nb == 1)
 * broadcasts against the other; n_out = max(na, nb).
 *   TRK_FRAME_COMPOSE      out = a o b       Frame.multiply_transform     frame.py:64-68, geometrics/utils.py:11-17
 *   TRK_FRAME_INVERSE      out = a^-1        Frame.inverse                frame.py:57-62  (b ignored)
 *   TRK_FRAME_INV_COMPOSE  out = b^-1 o a    Frame.multiply_inv_transform frame.py:70-76, geometrics/utils.py:21-29 */
#define TRK_FRAME_COMPOSE 0
#define TRK_FRAME_INVERSE 1
#define TRK_FRAME_INV_COMPOSE 2
int trk_frame_compose(int32_t op, const float* Ra, const float* ta, int64_t na, const float* Rb, const float* tb, int64_t nb,
                      float* R_out, float* t_out, trk_stream_t stream);
/* Reverse mode of the above for equal batch sizes (a broadcast input is expanded by the caller): (gR, gt) [n] ->
 * gRa, gta [n] and -- unless op is TRK_FRAME_INVERSE -- gRb, gtb [n]. */
int trk_frame_compose_backward(int32_t op, const float* Ra, const float* ta, const float* Rb, const float* tb, const float* gR,
                               const float* gt, int64_t n, float* gRa, float* gta, float* gRb, float* gtb, trk_stream_t stream);
/* Frame.transform_point frame.py:116-118: points [P,3] in the frames -> out [n,P,3] = R_s p + t_s (what fk_map_collision
 * does with a grasped object's points, robot_panda.py:154-168). */
int trk_frame_transform_points(const float* R, const float* t, int64_t n, const float* points, int32_t n_points, float* out,
                               trk_stream_t stream);
/* its reverse mode w.r.t. the poses: gout [n,P,3] -> gR [n,9] = sum_p g_p p^T, gt [n,3] = sum_p g_p */
int trk_frame_transform_points_backward(const float* gout, int64_t n, const float* points, int32_t n_points, float* gR,
                                        float* gt, trk_stream_t stream);
/* Frame.get_quaternion frame.py:87-114 (trace method; XYZW, the reference converts with q_convert_wxyz at
 * robot_tree.py:214-215) and Frame.get_euler frame.py:120-121 (roll, pitch, yaw).  R as in trk_rotmat_to_quat.
 * Either output may be NULL. */
int trk_frame_quat_euler(const float* R, int64_t n, int32_t stride, int32_t row_pitch, float* quat_xyzw, float* euler,
                         trk_stream_t stream);
/* Reverse mode of trk_frame_quat_euler w.r.t. the rotations: gquat_xyzw [n,4] and / or geuler [n,3] (either may be NULL)
 * -> gR [n,9] (packed).  Euler angles: the derivatives of torch.atan2 / torch.asin (frame.py:120-121).  Quaternion: the
 * reference multiplies its trace-method vector by the PYTHON float `0.5 / math.sqrt(tn * M[n,3,3])` (frame.py:112), which
 * autograd treats as a constant; the gradient here is the reference's: scale held fixed, branch as taken in the forward. */
int trk_frame_quat_euler_backward(const float* R, int64_t n, int32_t stride, int32_t row_pitch, const float* gquat_xyzw,
                                  const float* geuler, float* gR, trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Planning objectives ("cost model").  Host arrays, copied at create().
 * reference: torch_planning_objectives/fields/distance_fields.py, environments/primitives.py,
 *            environments/grid_map_sdf.py, robots/robot_base.py:105-141.
 * --------------------------------------------------------------------------------- */
typedef enum TrkPrimType {
    TRK_PRIM_SPHERE = 0,        /* MultiSphereField     primitives.py:108-112 */
    TRK_PRIM_ROUNDED_BOX = 1,   /* MultiBoxField        primitives.py:327-334 */
    TRK_PRIM_SHARP_BOX = 2      /* MultiSharpBoxField   primitives.py:220-223 */
} TrkPrimType;

typedef struct TrkPrimitive {
    int32_t type;               /* TrkPrimType */
    int32_t object;             /* index into objects[] */
    float center[3];
    float half[3];              /* boxes: sizes/2 */
    float radius;               /* sphere radius, or rounded-box rounding radius (0.15*min size) */
    float _pad;
} TrkPrimitive;

typedef struct TrkObject {      /* ObjectField pose, primitives.py:387-405: p' = R^T (p - pos) */
    float pos[3];
    float R[9];                 /* q_to_rotation_matrix(ori), row-major */
    int32_t prim_begin;         /* primitives [prim_begin, prim_end) belong to this object */
    int32_t prim_end;
    int32_t is_grid;            /* 1: this "object" is the precomputed grid (GridMapSDF) */
    int32_t _pad;
} TrkObject;

typedef struct TrkGridDesc {    /* GridMapSDF grid_map_sdf.py:9-117 (device pointers, caller-owned).  trk_cost_model_create packs
                                   the two arrays into its own (grad, sdf) records on the stream-0 timeline: like the host
                                   tables the grid is a snapshot taken at create(), later writes to sdf / grad are not seen */
    const float* sdf;           /* DEVICE [nx,ny,nz] */
    const float* grad;          /* DEVICE [nx,ny,nz,3] */
    int32_t dims[3];
    float lim_min[3];
    float map_dim[3];           /* |lim_max - lim_min| */
} TrkGridDesc;

typedef struct TrkCostModelDesc {
    int32_t abi_version;
    int32_t n_links_in;         /* links per sample in the position tensors handed to the cost ops */
    /* objects + workspace fields (CollisionObjectDistanceField / ...WorkspaceBoundaries...) */
    int32_t n_obj_links;        /* Lc */
    const int32_t* obj_link_idx;    /* [Lc] index into the position tensor */
    const float* obj_link_margin;   /* [Lc] collision_margins + cutoff_margin, added in fp32 on the host
                                       exactly as distance_fields.py:112 does */
    int32_t n_objects;
    const TrkObject* objects;
    int32_t n_prims;
    const TrkPrimitive* prims;
    int32_t has_grid;
    TrkGridDesc grid;
    int32_t has_ws;
    float ws_min[3];
    float ws_max[3];
    /* self collision (CollisionSelfField distance_fields.py:180-215) */
    int32_t n_self_links;       /* Ls */
    const int32_t* self_link_idx;   /* [Ls] index into the position tensor */
    int32_t n_self_pairs;       /* P */
    const int32_t* self_pairs;      /* [P*2] indices into self_link_idx.  A pair (a, a) is the reference's single-link case
                                       (distance_fields.py:195-198): "distance" 1e9 * |p_a|_1, so cost = margin - 1e9 |p_a|_1 */
    const float* self_margin;       /* [P] */
    /* end-effector SE(3) tracking (EESE3DistanceField distance_fields.py:335-359) */
    int32_t ee_link;            /* link whose pose is tracked (fused op); -1 = none */
    float ee_w_pos;
    float ee_w_rot;
    int32_t ee_square;
    float ee_target[16];        /* default target, row-major 4x4 */
    /* a second tracked link with its own target, same weights / square flag (two-arm scenes: BASELINE config 5 tracks
     * "EE on both arms"; the reference would sum two EESE3DistanceFields).  -1 = none. */
    int32_t ee2_link;
    float ee2_target[16];
    /* clamp_sdf=True of the fields (distance_fields.py:114-117): TRK_FIELD_* mask of the fields whose per-link (per-pair)
     * terms are relu(margin - signed distance) instead of margin - signed distance -- the hinge form planners optimise */
    int32_t clamp_fields;
    /* interpolate_link_pos=True of the embodiment fields (interpolate_points_v1 distance_fields.py:66-69, used at :145-147):
     * n_virtual extra position columns behind the n_links_in given ones,
     *     column n_links_in + k = virtual_w[2k] * column virtual_src[2k] + virtual_w[2k+1] * column virtual_src[2k+1],
     * which obj_link_idx / self_link_idx may name like any other column (0 <= index < n_links_in + n_virtual).  The table is
     * F.interpolate(mode='linear', align_corners=True) unrolled on the host: source columns and fp32 weights per output
     * point.  Position tensors handed to the cost ops keep n_links_in columns; gradients are scattered back to them. */
    int32_t n_virtual;              /* <= TRK_MAX_VIRTUAL */
    const int32_t* virtual_src;     /* [2*n_virtual] real columns (< n_links_in) */
    const float* virtual_w;         /* [2*n_virtual] */
} TrkCostModelDesc;

typedef struct TrkCostModel TrkCostModel;

int trk_cost_model_create(const TrkCostModelDesc* desc, TrkCostModel** out);
void trk_cost_model_destroy(TrkCostModel* cm);
/* reference: EESE3DistanceField.update_target distance_fields.py:344-345.  Host pointer, 16 floats. */
int trk_cost_model_set_ee_target(TrkCostModel* cm, const float* H16);
int trk_cost_model_set_ee2_target(TrkCostModel* cm, const float* H16);
/* trk_cost_fields may run a generated unit's field kernel when the cost model's columns and link sets equal a unit's collision
 * template (default: on); off = always the table-driven kernel (A/B tests). */
int trk_cost_model_enable_specialized(TrkCostModel* cm, int32_t on);

/* Which field a cost op evaluates. */
typedef enum TrkField {
    TRK_FIELD_SELF = 1,         /* CollisionSelfField */
    TRK_FIELD_OBJECTS = 2,      /* CollisionObjectDistanceField (analytic objects and/or grid) */
    TRK_FIELD_WS = 4            /* CollisionWorkspaceBoundariesDistanceField */
} TrkField;

/* reference: EmbodimentDistanceFieldBase.compute_embodiment_cost (field_type='sdf')
 *            distance_fields.py:107-124 for the fields in `fields` (bit-or of TrkField):
 *            cost[n] = sum over selected fields of  sum_links max_objects (margin - sdf).
 * link_pos [N, n_links_in, 3] -> cost [N].  g_link_pos (nullable) [N, n_links_in, 3] receives
 * d(sum_n gcost[n]*cost[n])/d link_pos (gcost NULL = ones): forward and explicit backward in
 * one pass, because the gradient is a by-product of the arg-min search. */
int trk_cost_fields(const TrkCostModel* cm, int32_t fields, const float* link_pos, int64_t n,
                    const float* gcost, float* cost, float* g_link_pos, trk_stream_t stream);

/* reference: compute_embodiment_collision (field_type='occupancy') distance_fields.py:210-215,
 *            283-291; PlanningTask ORs the fields tasks.py:227-228.
 * margin_override: NaN = per-link/per-pair default margins, else the scalar `margin=` kwarg.
 * -> in_collision [N] (uint8 0/1). */
int trk_collision_fields(const TrkCostModel* cm, int32_t fields, const float* link_pos, int64_t n,
                         float margin_override, uint8_t* in_collision, trk_stream_t stream);

/* reference: EESE3DistanceField.compute_costs_impl distance_fields.py:347-356 + SE3_distance
 *            geometrics/utils.py:130-154.
 * H_ee: n transforms `stride` floats apart (e.g. the last link of [N,L,4,4]: pointer offset
 * (L-1)*16, stride L*16).  target: DEVICE [16] (per_sample_target=0) or [N,16] (=1); NULL = the
 * cost model's stored target.  -> cost [N]; gH (nullable), same layout as H_ee, receives
 * gcost[n]*dcost/dH (gcost NULL = ones; all 16 floats of each transform are written, the constant
 * bottom row as zeros; other links' blocks of a strided gH are untouched). */
int trk_ee_cost(const TrkCostModel* cm, const float* H_ee, int64_t n, int64_t stride,
                const float* target, int32_t per_sample_target,
                const float* gcost, float* cost, float* gH, int64_t g_stride, trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Fused rollout: FK -> costs -> d cost / d q in one kernel (the north-star path).
 * reference chain replaced: PlanningTask.compute_collision_cost tasks.py:135-137,206-230
 *   (RobotPanda.fk_map_collision + the three collision fields) + EESE3DistanceField
 *   + `cost.sum().backward()`.
 * q [B,H,D] -> link_pos_out (nullable) [B,H,L,3], cost [B,H], gq [B,H,D];
 * cost = w_self*self + w_obj*objects + w_ws*workspace + w_ee*ee  (a zero weight skips the term);
 * gq = d cost[b,h] / d q[b,h,:] (samples are independent, so this equals the gradient of
 * cost.sum()).  cost_block_sums (nullable): DEVICE float[ceil(B*H/64)]; entry w receives the sum of
 * cost over samples [64w, 64w+64) -- one wave-level reduction and one plain store per wavefront, no
 * atomics, bit-reproducible.  With horizon 64 these are the per-trajectory costs; trk_reduce_sum folds
 * them into the scalar a multi-GPU caller all-reduces.
 * The cost model's link indices refer to the robot's L links (n_links_in == L).
 * --------------------------------------------------------------------------------- */
typedef struct TrkRolloutWeights {
    float w_self, w_obj, w_ws, w_ee;
} TrkRolloutWeights;

int trk_rollout_cost_grad(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* w,
                          const float* q, int64_t batch, int32_t horizon,
                          float* link_pos_out, float* cost, float* gq, float* cost_block_sums,
                          trk_stream_t stream);

/* BASELINE config 4's step -- "FK + Jacobian + cost" -- as ONE call: trk_rollout_cost_grad plus the stateful FK + geometric Jacobian
 * of `link` (trk_fk_jacobian without velocities: pos [N,3], quat_wxyz [N,4], lin_jac / ang_jac [N,3,D], N = batch*horizon).
 * reference: PlanningTask._compute_collision_or_cost tasks.py:139-232 followed by
 * DifferentiableTree.compute_forward_kinematics_and_geometric_jacobian robot_tree.py:218-248 on the same q.
 * ONE launch when a generated unit serves the cost model, `link` is the unit's tracked link, link_pos_out is given and the stateful
 * walk coincides with the stateless one on the columns' chains (UR10 + Allegro: the Jacobian columns are read out of the poses the
 * rollout already holds -- no second walk, q read once); otherwise the two launches, same results (trk_last_dispatch tells). */
int trk_rollout_jacobian_cost_grad(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* w, const float* q,
                                   int64_t batch, int32_t horizon, int32_t link, float* link_pos_out, float* cost, float* gq,
                                   float* cost_block_sums, float* pos, float* quat_wxyz, float* lin_jac, float* ang_jac,
                                   trk_stream_t stream);

/* 1 when trk_rollout_cost_grad(model, cm, w, ...) is served by a generated (model-specialised) kernel -- one whose baked
 * collision template equals the cost model's link sets for the terms `w` selects --, 0 when the table-driven kernel would run
 * (~10 x slower).  A deployment that must not fall back silently asserts this once after building its handles. */
int trk_rollout_is_specialized(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* w);

/* Which kernel family served the CALLING THREAD's latest rollout call (trk_rollout_cost_grad[_f16], trk_rollout_gp_cost_grad,
 * trk_rollout_points_cost_grad, trk_rollout_collision[_via], trk_rollout_points_collision[_via], trk_rollout_via_cost_grad, trk_rollout_gp_via_adam_steps).  No reference counterpart: the reference has one code path
 * (tasks.py:139-232); here a cost model whose link sets no generated unit bakes is served by the table-driven kernels, 10 - 30 x slower. */
enum {
    TRK_DISPATCH_NONE = 0,                  /* no rollout call yet on this thread (or a call that had nothing to launch) */
    TRK_DISPATCH_GENERATED = 1,             /* one launch of a generated (model-specialised) kernel */
    TRK_DISPATCH_TABLE = 2,                 /* the table-driven kernels */
    TRK_DISPATCH_GENERATED_PLUS_PRIOR = 3,  /* trk_rollout_gp_cost_grad: generated rollout, the GP prior as launches of its own;
                                             * trk_rollout_jacobian_cost_grad: generated rollout, the Jacobian as a launch of its own */
    TRK_DISPATCH_GENERATED_VIA_COST = 4,    /* trk_rollout_via_cost_grad: one launch of the generated via-point cost kernel */
    TRK_DISPATCH_GENERATED_VIA_ADAM = 5     /* trk_rollout_gp_via_adam_steps: the generated planning-loop kernel with the via-point term */
};
int trk_last_dispatch(void);
/* The generated rollout kernels come in two families: the generic one, and a plan-specialised one that has the objective terms with
 * non-zero weight, the requested outputs and the scene's sphere-pair count compiled in (fp32 I/O, identity base, a scene of <= 16
 * equal spheres; a collision point the model holds at a constant position is evaluated once per cost model and unit instead of per
 * sample).  Both compute the same values; trk_last_dispatch answers TRK_DISPATCH_GENERATED for either.
 * trk_last_plan_specialized: 1 when this thread's latest trk_rollout_cost_grad launch ran a plan-specialised kernel, else 0.
 * trk_set_plan_specialized (process-wide, default on): 0 keeps every launch on the generic family.  Returns the previous setting. */
int trk_last_plan_specialized(void);
int trk_set_plan_specialized(int on);
/* trk_rollout_is_specialized for trk_rollout_points_cost_grad(ps->model, ps, cm, w, ...) (16-byte aligned point_pos_out assumed). */
int trk_rollout_points_is_specialized(const TrkPointSet* ps, const TrkCostModel* cm, const TrkRolloutWeights* w);
/* Strict mode (process-wide; also TRK_STRICT_SPECIALIZED=1 in the environment, read once): the rollout entry points above return
 * TRK_ERR_UNSUPPORTED instead of launching a table-driven kernel when the model HAS generated units but none matches the call.
 * Models without any generated unit are served as before.  Returns the previous setting. */
int trk_set_strict_specialized(int on);
/* A weight on a term the cost model does not have (w_self without self pairs, w_ws without a workspace box, w_obj on an empty
 * scene, w_ee without a tracked link) contributes nothing in either kernel family and never influences the dispatch. */

/* Registers a generated unit that was compiled to a CODE OBJECT in-process (torch_robotics_amd/jit.py: hipRTC, the fall-back when
 * no hipcc is installed) -- the unit's device half only; libtrk.so's generic launchers play its host half.  Used by the package's
 * run-time compiler, not by applications.  code: the code object (kept mapped by the HIP module); name_exprs / lowered_names
 * [n_kernels]: the kernels' C++ name expressions (as codegen.py lists them) and their mangled names; the *_ok / chunked /
 * fast_switch / jac_direct flags and the layout stamp come from the generator and the headers the object was compiled with
 * (a stamp of another layout is refused). */
typedef struct TrkModuleUnitDesc {
    int32_t spec_abi_version;
    uint32_t sizeof_args, sizeof_cost_hdr;
    const char* ident;
    uint64_t model_hash;
    int32_t n_links, n_dofs;
    int32_t n_obj_links; const int32_t* obj_link_idx;
    int32_t n_self_pairs; const int32_t* self_pairs;          /* [2 * n_self_pairs] LINK indices */
    int32_t ee_link, ee2_link;
    int32_t n_virtual; const int32_t* virtual_src; const float* virtual_w;
    int32_t chunked, fast_switch, fkhbwd_ok, fields_ok, ik_ok, ikgn_ok, jac_ok, jac_direct, gp_ok;
    const void* code; uint64_t code_size;
    int32_t n_kernels; const char* const* name_exprs; const char* const* lowered_names;
    /* n_points > 0: an ATTACHED-POINT unit (link spheres, grasped-object points): obj_link_idx / self_pairs are COLUMN indices of the
     * point set, points_hash identifies it (codegen.points_hash); its kernels are the fused rollout and the positions' reverse mode */
    int32_t n_points; uint64_t points_hash;
} TrkModuleUnitDesc;
int trk_spec_register_module(const TrkModuleUnitDesc* desc);
/* The layout stamp the generated units of this library carry (TRK_SPEC_ABI_VERSION, sizeof(SpecArgs) + sizeof(IkArgs) +
 * sizeof(IkGnArgs), sizeof(DevCostHdr)): what a TrkModuleUnitDesc must repeat.  out [3]. */
int trk_spec_layout_stamp(int64_t* out);

/* Fused FK + boolean collision fields: q [batch*horizon, D] -> in_collision [batch*horizon] (1 = at least one selected field
 * has a signed distance below its margin).  No link positions, costs or gradients are written.
 * reference: PlanningTask.compute_collision tasks.py:131-133 -> _compute_collision_or_cost(field_type='occupancy') tasks.py:139-232
 * = fk_map_collision (robot_base.py:171-174) + the OR of the fields' compute_embodiment_collision (distance_fields.py:210-215,
 * 283-291); get_trajs_collision_and_free calls it with margin=0. on the interpolated via points (tasks.py:247-251).
 * margin_override: NaN = each field's own margins (per-link margin + cutoff, per-pair margin), else this margin for every test.
 * link_pos_ws: DEVICE scratch [N, L, 3], used only when no generated kernel serves this model / cost model (then the
 * table-driven FK and field kernels run back to back); may be NULL otherwise. */
int trk_rollout_collision(const TrkModel* model, const TrkCostModel* cm, int32_t fields, const float* q, int64_t batch,
                          int32_t horizon, float margin_override, uint8_t* in_collision, float* link_pos_ws,
                          trk_stream_t stream);

/* element types of the reduced-precision entry points */
#define TRK_F32 0
#define TRK_F16 1

/* trk_rollout_cost_grad with q and link_pos_out stored as IEEE fp16 in HBM -- BASELINE config 5's "fp16 with fp32
 * cost accumulate": arithmetic, `cost` and `cost_block_sums` stay fp32; inputs are widened and outputs rounded once
 * (round-to-nearest-even) at the memory boundary.  Build-defined (the reference has no reduced-precision path); the
 * check is the fp64 oracle on the same fp16-rounded q.
 * The gradient: gq [B,H,D] of grad_dtype (TRK_F16, or TRK_F32 = the mixed mode: fp16 trajectories and positions, fp32
 * gradient) receives grad_scale * d cost / d q, the product formed in fp32; an fp16 store SATURATES at +-65504 -- it never
 * writes inf.  grad_scale (> 0, a power of two keeps the mantissa) is the caller's loss scale: the GP prior this gradient
 * is summed with (trk_gp_prior_cost_grad, same scale) reaches 1e5 .. 1e6 at config 5's sigma_gp = 0.1, dt = 5/128
 * (env_spheres_3d.py:57), beyond the fp16 range; the consumer divides by the scale (or folds it into its step size). */
int trk_rollout_cost_grad_f16(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* w,
                              const void* q_f16, int64_t batch, int32_t horizon, void* link_pos_out_f16, float* cost,
                              void* gq, int32_t grad_dtype, float grad_scale, float* cost_block_sums, trk_stream_t stream);

/* BASELINE config 5's objective in ONE launch: trk_rollout_cost_grad(_f16) and the GP prior (trk_gp_prior_cost_grad) fused -- the
 * trajectory's q / qd rows are read once, gq and gqd are written once (no read-modify-write of the gradient between two launches).
 * BUILD-DEFINED like its two halves; checked against the fp64 oracle of both.
 *   q, qd [B,H,D] of io_dtype (TRK_F32 / TRK_F16; samples of a trajectory are consecutive, `horizon` of them);
 *   cost [B,H] (fp32) = the rollout's cost + weight/2 e_t^T Q^-1 e_t, the prior's factor between t and t+1 attributed to
 *       sample t (0 at t = H-1): sum_t cost[b,t] = the rollout's total + trk_gp_prior_cost_grad's cost[b];
 *   gq [B,H,D] = grad_scale (d rollout cost / d q + d prior / d q),  gqd [B,H,D] = grad_scale d prior / d qd, both of grad_dtype
 *       (fp16 stores saturate; fp32 trajectories: fp32 gradients, grad_scale = 1);  link_pos_out (nullable) [B,H,L,3] of io_dtype;
 *   cost_block_sums (nullable): as trk_rollout_cost_grad, of the combined cost.
 * A generated unit serves it with its subtrees scheduled one after the other (the dual Panda's arms: 128 registers, one resident
 * generation of wavefronts); where no unit does -- no unit for the robot, ring-staged robots, self pairs between the subtrees
 * with w_self != 0 -- the same result comes from the two-launch form (rollout, then the prior accumulated into its outputs). */
typedef struct TrkGpPrior {
    float dt, sigma, weight;
} TrkGpPrior;
int trk_rollout_gp_cost_grad(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* w, const TrkGpPrior* gp,
                             const void* q, const void* qd, int64_t batch, int32_t horizon, int32_t io_dtype,
                             void* link_pos_out, float* cost, void* gq, void* gqd, int32_t grad_dtype, float grad_scale,
                             float* cost_block_sums, trk_stream_t stream);

/* trk_rollout_cost_grad with the collision fields evaluated on attached points instead of link origins: the cost
 * model's position columns (n_links_in, obj_link_idx, self_link_idx) index the points of `ps`; ee_link stays a LINK
 * index of the model.  point_pos_out [batch*horizon, n_points, 3] (nullable).  Same outputs otherwise. */
int trk_rollout_points_cost_grad(const TrkModel* model, const TrkPointSet* ps, const TrkCostModel* cm,
                                 const TrkRolloutWeights* w, const float* q, int64_t batch, int32_t horizon,
                                 float* point_pos_out, float* cost, float* gq, float* cost_block_sums,
                                 trk_stream_t stream);

/* reference: interpolate_traj_via_points trajectory/utils.py:37-50 (used by PlanningTask.get_trajs_collision_and_free
 * tasks.py:234-251): x [T, H, D] -> out [T, (H-1)*n_interp, D], out[t, i*n+a] = x[t,i]*alpha[a] + x[t,i+1]*beta[a];
 * alpha = linspace(0,1,n+2)[1:n+1], beta = 1 - alpha: DEVICE float[n_interp], computed by the caller. */
int trk_interpolate_via_points(const float* x, int64_t n_traj, int32_t horizon, int32_t dim, int32_t n_interp,
                               const float* alpha, const float* beta, float* out, trk_stream_t stream);

/* Trajectory validation in one pass over the via points: trk_interpolate_via_points + trk_rollout_collision without the
 * interpolated trajectories ever reaching HBM.  x [n_traj, horizon, state_dim] (the first D columns of a way point are the joint
 * positions, robot_base.py:148-149); sample (t, i, a) is x[t, i] * alpha[a] + x[t, i + 1] * beta[a], products and sum each rounded
 * once (trajectory/utils.py:47-49) -> in_collision [n_traj * (horizon - 1) * n_interp].
 * reference: PlanningTask.get_trajs_collision_and_free tasks.py:244-251 (margin_override = 0 there).
 * Served by the generated kernels only: TRK_ERR_UNSUPPORTED when no unit matches the model / cost model -- the caller then
 * runs the two-step form. */
int trk_rollout_collision_via(const TrkModel* model, const TrkCostModel* cm, int32_t fields, const float* x, int64_t n_traj,
                              int32_t horizon, int32_t state_dim, int32_t n_interp, const float* alpha, const float* beta,
                              float margin_override, uint8_t* in_collision, trk_stream_t stream);

/* The same launch also folds the per-trajectory FLAGS of trk_traj_validate (round 6) -- bit 0 = some interpolated configuration of the
 * trajectory collides (tasks.py:255-256), bit 1 = some joint position x[t, h, d < D] lies outside [q_min[d], q_max[d]] (DEVICE float[D];
 * NaN = outside; tasks.py:270-273; every way point is an end of some segment the kernel has loaded anyway) -- as per-WAVEFRONT partial
 * results: partial_flags [trk_via_partial_flags_bytes(n_traj, horizon, n_interp)] uint8, a row of hi / 64 + 2 bytes per trajectory
 * (hi = (horizon - 1) n_interp samples), one byte per wavefront of 64 consecutive samples that holds samples of it; every byte a reader
 * looks at is written by plain stores on every call (no atomics, nothing to zero).  Hand the buffer to trk_traj_validate as `waypoint_collisions` with n_waypoints = -(horizon - 1) * n_interp: its partition
 * launch ORs the few bytes that cover a trajectory, and the separate flags launch disappears. */
int64_t trk_via_partial_flags_bytes(int64_t n_traj, int32_t horizon, int32_t n_interp);
int trk_rollout_collision_via_flags(const TrkModel* model, const TrkCostModel* cm, int32_t fields, const float* x, int64_t n_traj,
                                    int32_t horizon, int32_t state_dim, int32_t n_interp, const float* alpha, const float* beta,
                                    float margin_override, const float* q_min, const float* q_max, uint8_t* in_collision,
                                    uint8_t* partial_flags, trk_stream_t stream);

/* trk_rollout_collision for a cost model whose columns are the attached points of `ps` (link spheres, grasped-object points; the model
 * is ps's): FK + the OR of the selected fields' tests in ONE launch, one byte per sample out, no point position reaches HBM.
 * reference: PlanningTask.compute_collision tasks.py:131-133 with such a robot.  Same validation and margin rule as
 * trk_rollout_collision; a field with nothing to test is dropped from the mask.  Served by the boolean kernels of a generated
 * attached-point unit (compiled ahead of time or by hipcc at run time; a unit loaded as a code object has none).  Without one: the
 * two launches trk_fk_points + trk_collision_fields through point_pos_ws [batch*horizon, n_points, 3] (TRK_ERR_INVALID_ARG when it is
 * NULL; TRK_ERR_UNSUPPORTED in strict mode when the point set has generated kernels).  trk_last_dispatch tells which. */
int trk_rollout_points_collision(const TrkPointSet* ps, const TrkCostModel* cm, int32_t fields, const float* q, int64_t batch,
                                 int32_t horizon, float margin_override, uint8_t* in_collision, float* point_pos_ws,
                                 trk_stream_t stream);

/* trk_rollout_collision_via / _via_flags for such a cost model: the via points are interpolated in the kernel (reference:
 * PlanningTask.get_trajs_collision_and_free tasks.py:244-251).  traj_flags, q_min and q_max are given together (the per-wavefront
 * partial flags of trk_rollout_collision_via_flags, trk_via_partial_flags_bytes(n_traj, horizon, n_interp) bytes, ready for
 * trk_traj_validate) or all NULL.  Served by the generated boolean kernels only: TRK_ERR_UNSUPPORTED when none serves the point
 * set / cost model -- the caller then runs trk_interpolate_via_points + trk_rollout_points_collision. */
int trk_rollout_points_collision_via(const TrkPointSet* ps, const TrkCostModel* cm, int32_t fields, const float* x, int64_t n_traj,
                                     int32_t horizon, int32_t state_dim, int32_t n_interp, const float* alpha, const float* beta,
                                     float margin_override, const float* q_min, const float* q_max, uint8_t* in_collision,
                                     uint8_t* traj_flags, trk_stream_t stream);

/* The rest of get_trajs_collision_and_free (tasks.py:253-299) on the device: three launches, no host round trip (two when
 * `waypoint_collisions` is the partial_flags buffer of trk_rollout_collision_via_flags and n_waypoints = -(samples per trajectory):
 * the partition launch assembles flags [n_traj] itself; q_min / q_max are then unused).
 *   flags [n_traj]      bit 0: some way-point byte of the trajectory is set (waypoint_collisions [n_traj, n_waypoints]);
 *                       bit 1: some joint position x[t, h, d < n_dofs] lies outside [q_min[d], q_max[d]] (NaN = outside)
 *   idx [n_traj rows]   a stable three-way partition of the trajectories, each group in increasing order:
 *                         rows [0, n_free)              flags == 0: collision free and inside the limits (tasks.py:255, 274, 282)
 *                         rows [n_free, +n_coll)        bit 0 set: colliding                             (tasks.py:256)
 *                         rows [.., +n_out)             flags == 2: collision free, outside the limits   (tasks.py:278-281)
 *                       int64 rows [t] (inner == 0) or [t / inner, t % inner] (a 4-D batch [n_traj / inner, inner, ...]),
 *                       like torch.argwhere.  The reference's `trajs_coll_idxs` is the last two groups together.
 *   counts [4]          DEVICE {n_free, n_coll, n_out, ticket}.  counts_host (nullable): PINNED HOST int32[4] that receives the
 *                       same numbers straight from the kernel (device-addressable under unified addressing), the ticket last
 *                       with system-scope release semantics: the host polls counts_host[3] for the `ticket` it passed -- no
 *                       copy call, no event -- and that is the only device -> host traffic of a validation.
 *   gathered (nullable) [n_traj, horizon, state_dim]: gathered[r] = x[idx[r]] (free trajectories first, then the others). */
int trk_traj_validate(const uint8_t* waypoint_collisions, const float* x, int64_t n_traj, int32_t horizon, int32_t state_dim,
                      int32_t n_waypoints, int32_t n_dofs, const float* q_min, const float* q_max, int64_t inner,
                      uint8_t* flags, int64_t* idx, int32_t* counts, int32_t* counts_host, int32_t ticket, float* gathered,
                      trk_stream_t stream);

/* reference: interpolate_points_v1 distance_fields.py:66-69 = F.interpolate(points^T, size=n_out, mode='linear',
 * align_corners=True)^T along the link axis (the link-sphere approximation of interpolate_link_pos, :145-147; also used by
 * robot_panda.py:199).  x [N, n_in, channels] -> out [N, n_out, channels],
 *     out[n, k, :] = w[2k] * x[n, src[2k], :] + w[2k+1] * x[n, src[2k+1], :];
 * src / w: DEVICE int32 / float [2 * n_out] -- ATen's source indices and fp32 weights, computed by the caller
 * (torch_robotics_amd/costmodel.py: interpolation_table).  _backward: gout [N, n_out, channels] -> gx [N, n_in, channels]. */
int trk_interpolate_columns(const float* x, int64_t n, int32_t n_in, int32_t channels, int32_t n_out, const int32_t* src,
                            const float* w, float* out, trk_stream_t stream);
int trk_interpolate_columns_backward(const float* gout, int64_t n, int32_t n_in, int32_t channels, int32_t n_out,
                                     const int32_t* src, const float* w, float* gx, trk_stream_t stream);

/* Constant-velocity Gaussian-process prior over trajectories -- the "GP-smoothness" term of BASELINE config 5.
 * BUILD-DEFINED, parity unpinned: the reference contains no such cost (its smoothness is finite differences,
 * trajectory/utils.py:53-64, metrics.py:27-35; it only carries the hyper-parameter names sigma_gp, dt for external
 * planners, env_spheres_3d.py:51-76).  The standard GPMP form is used:  per DOF x_t = (q_t, qd_t),
 * e_t = Phi(dt) x_t - x_{t+1},  Q^-1 = sigma^-2 [[12/dt^3, -6/dt^2], [-6/dt^2, 4/dt]],
 * cost[b] = weight * 1/2 sum_t sum_dof e_t^T Q^-1 e_t   and   gq, gqd = d cost / d q, d cost / d qd.
 * q, qd: [batch, horizon, dof] of `io_dtype` (TRK_F32 / TRK_F16; arithmetic and `cost` are fp32); gq, gqd: the same shape
 * of `grad_dtype` (TRK_F32, or TRK_F16 with fp16 trajectories) and receive grad_scale * the gradient (product in fp32; an
 * fp16 store saturates at +-65504, see trk_rollout_cost_grad_f16; `cost` is not scaled).  accumulate != 0 adds into
 * gq / gqd instead of overwriting -- to compose with trk_rollout_cost_grad(_f16)'s gradient, written with the same scale.
 * fp16-stored q puts a quantisation floor under this term: ulp(q)^2 / 12 * 12 / (sigma^2 dt^3) per
 * residual -- ~1.6 per time step and joint at sigma = 0.1, dt = 5/128, |q| in [1, 2). */
int trk_gp_prior_cost_grad(const void* q, const void* qd, int64_t batch, int32_t horizon, int32_t dof, int32_t io_dtype,
                           float dt, float sigma, float weight, float* cost, void* gq, void* gqd, int32_t grad_dtype,
                           float grad_scale, int32_t accumulate, trk_stream_t stream);

/* reference: finite_difference_vector trajectory/utils.py:53-64 (RobotBase.get_velocity / get_acceleration
 * robot_base.py:151-166): zero-padded differences along the horizon.  x, out [batch, horizon, dim];
 * method 0 = forward, 1 = backward, 2 = central. */
int trk_finite_difference(const float* x, int64_t batch, int32_t horizon, int32_t dim, float dt, int32_t method,
                          float* out, trk_stream_t stream);
/* reference: compute_path_length / compute_smoothness trajectory/metrics.py:7-12, 27-35:
 * out[b] = sum_t || x[b, t+1, c0:c0+dim] - x[b, t, c0:c0+dim] ||, x [batch, horizon, state_dim]. */
int trk_traj_diff_norm_sum(const float* x, int64_t batch, int32_t horizon, int32_t state_dim, int32_t c0, int32_t dim,
                           float* out, trk_stream_t stream);

/* Gauss-Newton normal equations from the geometric Jacobian of one link (the output of trk_fk_jacobian; reference:
 * DifferentiableTree.compute_forward_kinematics_and_geometric_jacobian robot_tree.py:218-248 stops at lin_jac / ang_jac).
 * BUILD-DEFINED: per sample J = [lin_jac; ang_jac] (6 x D):  JtJ [n, D, D] = J^T J,  Jtr [n, D] = J^T residual (nullable;
 * residual [n, 6] = [linear(3), angular(3)]) -- what a damped least-squares / Gauss-Newton IK step solves (JtJ + lambda I) dq = Jtr.
 * use_mfma != 0 computes JtJ with v_mfma_f32_4x4x1_16b_f32 (dof <= 8) instead of per-lane FMAs: the same values to fp32 rounding;
 * both variants exist so that the two can be measured side by side (the op is HBM-bound).
 * dq (nullable) [n, D]: the damped step itself, (JtJ + lambda I) dq = Jtr solved per sample by a Cholesky factorisation in the
 * kernel (needs `residual`); damping: DEVICE lambda, [n] with damping_stride 1 or one value with damping_stride 0 (NULL: 0). */
int trk_jtj(const float* lin_jac, const float* ang_jac, const float* residual, int64_t n, int32_t dof, int32_t use_mfma,
            float* JtJ, float* Jtr, const float* damping, int32_t damping_stride, float* dq, trk_stream_t stream);

/* The chain rule of the fused rollout under autograd: out[n, :] = g[n, :] * scale[n * scale_stride] -- the saved
 * d cost[n] / d q[n, :] of trk_rollout_cost_grad times the upstream gradient of cost[n] (what
 * `PlanningTask.compute_collision_cost(q).sum().backward()`, tasks.py:135-137, asks of the op's backward).  g / out [n, dim] of
 * io_dtype (TRK_F32 / TRK_F16); scale fp32: [n] with scale_stride 1, or ONE value with scale_stride 0 (`.sum().backward()`
 * hands down an expanded scalar: no per-row tensor is materialised for it); out may be g. */
int trk_scale_rows(const void* g, const float* scale, int32_t scale_stride, int64_t n, int32_t dim, int32_t io_dtype, void* out,
                   trk_stream_t stream);

/* Profiling hook (process-global, NULL = off): DEVICE uint64[ceil(N/64)][8]; the model-specialised fused kernel then
 * records the shader clock (s_memtime) of every wavefront at 8 phase boundaries (entry, q loaded, FK done, positions
 * staged, objects done, objectives done, reverse done, exit).  Used by tools/phase_profile.py; never set in production. */
int trk_debug_set_stamp_buffer(void* device_u64);

/* The one buffer a batch-sharded planner all-reduces: packed [1 + H + H*D] =
 *   [ sum of all costs | sum over trajectories of cost(b, h) | sum over trajectories of gq(b, h, d) ]
 * of ONE rank's evaluation -- cost [batch, horizon], gq [batch, horizon, dof] and cost_block_sums as written by
 * trk_rollout_cost_grad -- bit-reproducibly (fixed association order; packed[0] equals trk_reduce_sum of the block sums; two
 * small launches: partial column sums of row slices, then their fold).  gq is of grad_dtype (TRK_F32, or TRK_F16: the gradient of trk_rollout_cost_grad_f16) and holds grad_scale x the
 * gradient; the fp32 column sums are divided by grad_scale once, so `packed` is always unscaled fp32.  traj_cost (nullable)
 * [batch]: a per-trajectory cost (trk_gp_prior_cost_grad's) whose sum is added to packed[0].
 * scratch: DEVICE memory of trk_pack_sums_scratch_bytes(horizon, dof) bytes (the partial rows); one scratch per stream that may
 * run the call concurrently. */
int64_t trk_pack_sums_scratch_bytes(int32_t horizon, int32_t dof);
int trk_pack_sums(const float* cost, const void* gq, int32_t grad_dtype, float grad_scale, const float* cost_block_sums,
                  const float* traj_cost, int64_t batch, int32_t horizon, int32_t dof, float* scratch, float* packed,
                  trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * The exchange step of a batch-sharded planner as a PEER-TO-PEER MAILBOX ("alternative = peer-to-peer write of
 * 8 partials + local sum"; what is sharded is PlanningTask._compute_collision_or_cost's batch, tasks.py:206-230; the reference
 * itself is single-device and has no exchange).  One process per GPU; every rank owns a mailbox in device memory with
 * n_slots x world rows of n_floats; trk_mailbox_exchange stores the caller's packed row (trk_pack_sums' output) into the
 * rank's row of EVERY mailbox (one xGMI hop, all peers in parallel), raises a sequence flag, waits for the `world` flags of
 * its own mailbox and writes the sum of the `world` rows, added in rank order (bit-identical on every rank and run), to out.
 * trk_mailbox_exchange = trk_mailbox_send (the stores and the flag: never waits) + trk_mailbox_recv (the wait and the sum); a
 * planner sends right after the evaluation whose sums travel and receives some evaluations later, when the peers' rows have
 * arrived -- the wait leaves the critical path without a second stream.  Single-workgroup kernels, asynchronous on `stream`;
 * the sequence numbers live in device memory, so the calls can be captured into a hipGraph and replayed.  All ranks must issue
 * the same sequence of exchanges, with EQUAL (world, n_floats, n_slots) on every rank (the offsets of a peer's rows follow from
 * them: exchange the triple with the handles and compare before connect); on one rank send k, recv k, send k + 1, ... run in
 * that (stream) order, with bounded look-ahead: send k + a may be issued before recv k only for a <= (n_slots - 2) / 2 (two
 * slots = strict alternation, four = one send ahead) -- a send beyond that is refused (TRK_ERR_INVALID_ARG), as is a recv without
 * a send (the host counts launches; a captured graph counts once and must therefore be balanced).  A rank that waits longer than
 * TRK_MAILBOX_TIMEOUT_S (environment, default 5 s) for a flag gives up, counts a time-out (sticky, trk_mailbox_status) and writes
 * NaN to every element of `out` -- never an incomplete sum -- instead of hanging the GPU.
 *   create:     allocates the local mailbox (uncached, else fine-grained, else plain device memory -- the first kind that
 *               hipIpcGetMemHandle accepts; TRK_MAILBOX_ALLOC=uncached|finegrained|plain in the environment forces one).
 *   ipc_handle: writes the TRK_MAILBOX_HANDLE_BYTES bytes another process passes to connect (exchange them with any host
 *               transport, e.g. torch.distributed.all_gather_object).
 *   connect:    handles [world][TRK_MAILBOX_HANDLE_BYTES] (HOST; the entry of this rank is ignored): maps the peers' mailboxes.
 *   status:     synchronises with the device; exchanges issued, time-outs seen, allocation kind (0 uncached, 1 fine-grained, 2 plain).
 * world == 1 needs no connect.  2 <= n_slots <= 64, world <= 16, n_floats <= 2^22. */
#define TRK_MAILBOX_HANDLE_BYTES 64
typedef struct TrkMailbox TrkMailbox;
int trk_mailbox_create(int32_t world, int32_t rank, int32_t n_floats, int32_t n_slots, TrkMailbox** out);
int trk_mailbox_ipc_handle(const TrkMailbox* mb, void* handle /* host, TRK_MAILBOX_HANDLE_BYTES */);
int trk_mailbox_connect(TrkMailbox* mb, const void* handles /* host */);
int trk_mailbox_send(TrkMailbox* mb, const float* packed, trk_stream_t stream);
int trk_mailbox_recv(TrkMailbox* mb, float* out, trk_stream_t stream);
int trk_mailbox_exchange(TrkMailbox* mb, const float* packed, float* out, trk_stream_t stream);
int trk_mailbox_status(const TrkMailbox* mb, int64_t* n_exchanges, int64_t* n_timeouts, int32_t* alloc_kind);
void trk_mailbox_destroy(TrkMailbox* mb);

/* What a pointer VALUE is to this library, without dereferencing it: 0 = not a live handle (never created here, or destroyed),
 * 1 = TrkModel, 2 = TrkCostModel, 3 = TrkPointSet.  For bindings that carry handles as integers (a PyTorch dispatcher op's schema
 * has tensors and scalars only, csrc/trk_torch_ops.cpp): a stale integer becomes an error instead of a segfault.  Thread-safe. */
int trk_handle_kind(const void* handle);

/* Deterministic sum of n floats (fixed association order, one workgroup): x [n] -> out [1]. */
int trk_reduce_sum(const float* x, int64_t n, float* out, trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * SDF grid precompute (GridMapSDF.precompute_sdf grid_map_sdf.py:34-63): evaluates the analytic
 * objects of `cm` and their gradient at the linspace voxel centres.
 * -> sdf [nx,ny,nz], grad [nx,ny,nz,3] (device, caller-allocated). */
int trk_grid_precompute(const TrkCostModel* cm, const int32_t dims[3], const float lim_min[3],
                        const float lim_max[3], float* sdf, float* grad, trk_stream_t stream);

/* Signed distance of arbitrary points to the cost model's objects:
 * reference: ObjectField.compute_signed_distance primitives.py:387-405 (per object) -> sdf [N, n_objects]
 * points [N,3]. grad (nullable) [N, n_objects, 3]. */
int trk_sdf_points(const TrkCostModel* cm, const float* points, int64_t n, float* sdf, float* grad,
                   trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * 2-D point mass in a planar scene (csrc/trk_planar.hip).
 * reference: RobotPointMass robot_point_mass.py:13-32 (identity "kinematics", one collision point) +
 *            PlanningTask tasks.py:131-232 with the object and workspace fields, distance_fields.py:107-130, 298-332,
 *            ObjectField in 2-D primitives.py:387-405, GridMapSDF in 2-D grid_map_sdf.py:34-114.
 * A sample is one point q = (x, y).  With m = the scene's margin (link margin + cutoff margin, added in fp32 on the host):
 *   objects:   max over the scene's df objects (the grid first, then the analytic objects in order) of (m - sdf_o(q)); an analytic
 *              object is the min over its primitives of the primitive's SDF at R(ori)^T ((x, y, 0) - pos), first two coordinates;
 *              the grid is the stored value of the nearest-lower cell floor((q - lim_min) / map_dim * dims), clamped to the grid.
 *   workspace: max over the four faces q - ws_min, ws_max - q (in that order) of (m - d); d/dq of sign(d) |d| is 0 at d == 0.
 *   cost = objects + workspace; clamp != 0 applies relu to both terms (clamp_sdf=True).  The gradient follows the first arg-max
 *   object and, inside it, the first arg-min primitive; a grid cell contributes its stored gradient.
 * --------------------------------------------------------------------------------- */
#define TRK_PLANAR_MAX_OBJECTS 64
#define TRK_PLANAR_MAX_PRIMS 256

typedef struct TrkPrim2D {      /* TrkPrimType; center / half sizes in the object frame; sphere radius or rounding radius */
    int32_t type;
    int32_t _pad;
    float center[2];
    float half[2];
    float radius;
    float _pad2;
} TrkPrim2D;

typedef struct TrkObject2D {    /* ObjectField: 3-D pos and q_to_rotation_matrix(ori) row-major, primitives [prim_begin, prim_end) */
    float pos[3];
    float R[9];
    int32_t prim_begin;
    int32_t prim_end;
} TrkObject2D;

typedef struct TrkScene2DDesc {
    int32_t abi_version;        /* TRK_ABI_VERSION */
    int32_t n_objects;          /* analytic objects (fixed objects without a grid, then the extra objects), <= TRK_PLANAR_MAX_OBJECTS */
    const TrkObject2D* objects; /* host */
    int32_t n_prims;            /* <= TRK_PLANAR_MAX_PRIMS */
    const TrkPrim2D* prims;     /* host */
    int32_t has_grid;           /* 1: the fixed objects are a precomputed grid (evaluated before the analytic objects) */
    int32_t grid_dims[2];
    const float* grid_cells;    /* DEVICE [nx, ny, 4] = (sdf, gx, gy, 0) as written by trk_grid2d_precompute; copied at create() */
    float grid_lim_min[2];
    float grid_map_dim[2];      /* |lim_max - lim_min| in fp32 */
    int32_t has_ws;
    float ws_min[2];
    float ws_max[2];
    float margin;               /* link margin + cutoff margin */
} TrkScene2DDesc;

typedef struct TrkScene2D TrkScene2D;

int trk_scene2d_create(const TrkScene2DDesc* desc, TrkScene2D** out);
void trk_scene2d_destroy(TrkScene2D* scene);

/* q [n, 2] -> cost [n]; grad (nullable) [n, 2] = d cost / d q.  clamp: relu of each term (clamp_sdf). */
int trk_scene2d_cost_grad(const TrkScene2D* scene, const float* q, int64_t n, int32_t clamp, float* cost, float* grad,
                          trk_stream_t stream);
/* any(sdf_o(q) < margin) over the objects and the workspace faces -> in_collision [n] (uint8 0 / 1).
 * margin_override: NaN = the scene's margin, else the `margin=` kwarg (tasks.py:131-133, distance_fields.py:283-291). */
int trk_scene2d_collision(const TrkScene2D* scene, const float* q, int64_t n, float margin_override, uint8_t* in_collision,
                          trk_stream_t stream);
/* trk_interpolate_via_points + trk_scene2d_collision in one launch (the interpolated points never reach memory): x [n_traj, horizon,
 * state_dim >= 2] -> in_collision [n_traj, (horizon - 1) * n_interp], sample (t, i, a) = x[t, i] * alpha[a] + x[t, i + 1] * beta[a]
 * rounded like trk_interpolate_via_points.  The result is trk_traj_validate's `waypoint_collisions`.  tasks.py:244-251. */
int trk_scene2d_collision_via(const TrkScene2D* scene, const float* x, int64_t n_traj, int32_t horizon, int32_t state_dim,
                              int32_t n_interp, const float* alpha, const float* beta, float margin_override,
                              uint8_t* in_collision, trk_stream_t stream);
/* GridMapSDF.precompute_sdf in 2-D (grid_map_sdf.py:34-63): the min over the scene's analytic objects and its gradient at the
 * torch.linspace grid points -> cells [dims[0], dims[1], 4] = (sdf, gx, gy, 0).  Ties between objects split the gradient evenly
 * (torch.minimum). */
int trk_grid2d_precompute(const TrkScene2D* scene, const int32_t dims[2], const float lim_min[2], const float lim_max[2],
                          float* cells, trk_stream_t stream);
/* Signed distance of points to each df object of the scene (the grid first, then the analytic objects):
 * points [n, 2] -> sdf [n, n_df], grad (nullable) [n, n_df, 2].  ObjectField / GridMapSDF.compute_signed_distance. */
int trk_scene2d_sdf_points(const TrkScene2D* scene, const float* points, int64_t n, float* sdf, float* grad, trk_stream_t stream);

/* The planners' trajectory objective of the 2-D point mass in ONE launch: trk_scene2d_cost_grad's hinge and the constant-velocity
 * GP prior (trk_gp_prior_cost_grad) with both gradients.  BUILD-DEFINED like the prior; the hinge half is the arithmetic of
 * trk_scene2d_cost_grad (bit for bit at w_obj = 1, gp.weight = 0), the prior half is checked against the fp64 oracle.
 *   q, qd [batch, horizon, 2] fp32, the samples of a trajectory consecutive; any horizon >= 1 (horizon 1 has no factor);
 *   cost [batch, horizon] = w_obj * (trk_scene2d_cost_grad's cost at q[b,t] with this clamp) + gp.weight/2 e_t^T Q^-1 e_t, the
 *       factor between t and t+1 attributed to sample t and 0 at t = horizon-1 (trk_rollout_gp_cost_grad's convention);
 *   gq [batch, horizon, 2] = w_obj d hinge / d q + d prior / d q,  gqd [batch, horizon, 2] = d prior / d qd; gq and gqd are
 *       nullable TOGETHER (cost only).  q, qd, gq, gqd 8-byte aligned. */
typedef struct TrkPlanarObjective {
    float w_obj;                /* finite */
    int32_t clamp;              /* relu of each hinge term (clamp_sdf) */
    TrkGpPrior gp;              /* dt > 0, sigma > 0, weight finite (0 = no prior) */
} TrkPlanarObjective;
int trk_scene2d_traj_cost_grad(const TrkScene2D* scene, const TrkPlanarObjective* objective, const float* q, const float* qd,
                               int64_t batch, int32_t horizon, float* cost, float* gq, float* gqd, trk_stream_t stream);

/* n_steps iterations of Adam (torch.optim.Adam's defaults, trk_ik_steps' arithmetic) on that objective with the trajectories and
 * the optimiser's state on the chip: q, qd [batch, horizon, 2] and adam_m, adam_v [batch, horizon, 4] = (q.x, q.y, qd.x, qd.y)
 * per sample are read once and written once per launch, at most 32 iterations per launch (more = several launches inside the
 * call; the result does not depend on how the iterations are grouped into calls).  Iterations first_step .. first_step +
 * n_steps - 1 are 1-based; adam_m / adam_v are zero before iteration 1.  Per component, with g its gradient:
 *   m1 = 0.9 m + 0.1 g,  v1 = 0.999 v + 0.001 g^2,  x -= (lr / bc1) * m1 / (sqrt(v1) / sqrt(bc2) + 1e-8),
 *   bc1 = 1 - 0.9^k and 1 / sqrt(bc2) = 1 / sqrt(1 - 0.999^k) formed in double on the host and rounded once to fp32.
 * pin: bit 1 q[:,0], 2 q[:,horizon-1], 4 qd[:,0], 8 qd[:,horizon-1] -- the gradient of a pinned component is taken as zero
 * (its value stays bit-unchanged, its m and v stay zero).  cost (nullable) [batch, horizon]: the objective of the state as
 * passed in.  lr = 0 (or n_steps = 0) only evaluates: nothing but cost is written.
 * 1 <= horizon <= TRK_PLANAR_MAX_HORIZON (one lane per sample, a workgroup owns whole trajectories): TRK_ERR_UNSUPPORTED above. */
#define TRK_PLANAR_MAX_HORIZON 256
typedef struct TrkPlanarAdam {
    float lr;                   /* finite */
    int32_t pin;                /* 0 .. 15 */
    int32_t first_step;         /* >= 1 */
    int32_t n_steps;            /* >= 0 */
} TrkPlanarAdam;
int trk_scene2d_traj_adam_steps(const TrkScene2D* scene, const TrkPlanarObjective* objective, const TrkPlanarAdam* adam, float* q,
                                float* qd, float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost,
                                trk_stream_t stream);

/* The same objective with the collision hinge ALSO at the via points that trajectory validation tests (trk_scene2d_collision_via):
 * v[b,i,a] = q[b,i] * alpha[a] + q[b,i+1] * beta[a] per coordinate, each product and the sum rounded once as in
 * trk_interpolate_via_points; alpha, beta DEVICE [n_interp].  With h, g the cost and gradient of trk_scene2d_cost_grad at a point:
 *   C[b,t] = sum_a h(v[b,t,a]),  L[b,t] = sum_a alpha[a] g(v[b,t,a]),  U[b,t] = sum_a beta[a] g(v[b,t,a])   (0 at t = horizon-1)
 *   cost[b,t] = (cost of trk_scene2d_traj_cost_grad) + w_via * C[b,t]           -- the segment t -> t+1 attributed to sample t
 *   gq[b,t]   = (gq of trk_scene2d_traj_cost_grad) + w_via * (L[b,t] + U[b,t-1]),  U[b,-1] = 0;   gqd is unchanged.
 * C adds in ascending a from 0, L and U are fmaf(weight, g, sum) in ascending a, then cost = fmaf(w_via, C, cost) and
 * gq = fmaf(w_via, L + U, gq): at w_via = 0, and at horizon 1 (no segment), the results are trk_scene2d_traj_cost_grad's.
 * One lane per sample, a workgroup owns whole trajectories: 1 <= horizon <= TRK_PLANAR_MAX_HORIZON for BOTH calls,
 * TRK_ERR_UNSUPPORTED above.  Everything else -- shapes, alignment, gq / gqd nullable together, cost nullable in the loop, pin,
 * first_step, 32 iterations per launch, lr = 0 -- is as in the two calls above.  No host synchronisation: capturable. */
typedef struct TrkPlanarViaObjective {
    TrkPlanarObjective base;    /* as trk_scene2d_traj_cost_grad validates it */
    float w_via;                /* finite */
    int32_t n_interp;           /* >= 1 */
    const float* alpha;         /* DEVICE [n_interp] */
    const float* beta;          /* DEVICE [n_interp] */
} TrkPlanarViaObjective;
int trk_scene2d_traj_via_cost_grad(const TrkScene2D* scene, const TrkPlanarViaObjective* objective, const float* q, const float* qd,
                                   int64_t batch, int32_t horizon, float* cost, float* gq, float* gqd, trk_stream_t stream);
int trk_scene2d_traj_via_adam_steps(const TrkScene2D* scene, const TrkPlanarViaObjective* objective, const TrkPlanarAdam* adam,
                                    float* q, float* qd, float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost,
                                    trk_stream_t stream);

/* The arm's planning loop on the chip: n_steps iterations of Adam (the arithmetic and bias terms of trk_scene2d_traj_adam_steps, above)
 * on the objective of trk_rollout_gp_cost_grad -- the collision and EE terms of trk_rollout_cost_grad under `w` plus the
 * constant-velocity GP prior -- with the trajectories and the optimiser's state in registers: q, qd [batch, horizon, dof] fp32 and
 * adam_m, adam_v [batch, horizon, 2 dof] = [q part | qd part] per sample are read once and written once per launch, at most 32
 * iterations per launch (more = several launches inside the call; the result does not depend on how the iterations are grouped into
 * calls).  pin: TrkPlanarAdam's bits.  cost (nullable) [batch, horizon]: the objective of the state as passed in, the prior's factor
 * t -> t+1 attributed to sample t.  lr = 0 (or n_steps = 0) only evaluates: nothing but cost is written.
 * Served by a generated kernel only (k_traj_adam: link-column units of robots up to 8 DOF); TRK_ERR_UNSUPPORTED when the horizon is
 * not a power of two <= TRK_TRAJ_ADAM_MAX_HORIZON (a wavefront owns whole trajectories), when no unit of the model carries the
 * kernel, when none matches the cost model, or when trk_model_enable_specialized is off.  No host synchronisation: capturable. */
#define TRK_TRAJ_ADAM_MAX_HORIZON 64
typedef struct TrkTrajAdam {
    float lr;                   /* finite */
    int32_t pin;                /* 0 .. 15 */
    int32_t first_step;         /* >= 1 */
    int32_t n_steps;            /* >= 0 */
} TrkTrajAdam;
int trk_rollout_gp_adam_steps(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* weights, const TrkGpPrior* gp,
                              const TrkTrajAdam* adam, float* q, float* qd, float* adam_m, float* adam_v, int64_t batch,
                              int32_t horizon, float* cost, trk_stream_t stream);

/* The collision / EE objective of trk_rollout_cost_grad at the via points BETWEEN the way points of a batch of trajectories, and its
 * gradient with respect to the way points, in one launch: nothing is materialised in between (reference:
 * interpolate_traj_via_points trajectory/utils.py:37-50 followed by the collision cost, differentiated through the interpolation).
 * x [n_traj, horizon, dof] fp32, contiguous (positions only).  Via point a of segment i is
 *   v[t, i, a] = x[t, i] * alpha[a] + x[t, i + 1] * beta[a],   0 <= i < horizon - 1, 0 <= a < n_interp,
 * each product and the sum rounded once (no FMA); alpha, beta: DEVICE [n_interp] (alpha = linspace(0, 1, n + 2)[1 : n + 1],
 * beta = 1 - alpha; a = 0 is the via point nearest x[t, i + 1]).
 *   cost (nullable) [n_traj, (horizon - 1) * n_interp]   cost[t, i * n_interp + a] = the objective at v[t, i, a]
 *   gq [n_traj, horizon, dof]                            gq[t, i] = sum_a seed[t, i, a] alpha[a] g(v[t, i, a])
 *                                                                 + sum_a seed[t, i - 1, a] beta[a] g(v[t, i - 1, a]),
 * g = the rollout's gradient with respect to the configuration; seed (nullable) [n_traj, (horizon - 1) * n_interp]: the upstream
 * gradient of every via point's cost, NULL = ones.  Every element of gq is written (no zeroing needed); the way points' own cost is
 * not part of this call (trk_rollout_cost_grad).  Bit-identical from run to run and however a batch is split into calls.
 * Validated before any device work; horizon < 2 or n_interp < 1: TRK_ERR_INVALID_ARG.  Served by a generated kernel only
 * (k_via_cost: link-column units of robots up to 8 DOF); TRK_ERR_UNSUPPORTED when horizon > TRK_VIA_COST_MAX_HORIZON (a wavefront owns
 * whole trajectories), when no unit of the model carries the kernel, when none matches the cost model, or when
 * trk_model_enable_specialized is off.  n_traj = 0: TRK_OK without a launch.  No host synchronisation: capturable. */
#define TRK_VIA_COST_MAX_HORIZON 64
int trk_rollout_via_cost_grad(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* weights, const float* x,
                              int64_t n_traj, int32_t horizon, int32_t n_interp, const float* alpha, const float* beta,
                              const float* seed, float* cost, float* gq, trk_stream_t stream);

/* trk_rollout_gp_adam_steps with the collision / EE objective ALSO at the via points that trajectory validation tests: the arm's
 * planning loop with the term of trk_rollout_via_cost_grad inside the kernel.  With h, g the weighted objective of
 * trk_rollout_cost_grad and its gradient at a configuration (the SAME `weights` at way points and via points) and
 *   v[b,t,a] = q[b,t] * alpha[a] + q[b,t+1] * beta[a]   (each product and the sum rounded once, as trk_rollout_via_cost_grad's),
 * the objective of an iteration is trk_rollout_gp_adam_steps' plus
 *   cost[b,t] += w_via * sum_a h(v[b,t,a])      -- the segment t -> t+1 attributed to sample t, 0 at t = horizon-1
 *   gq[b,t]   += w_via * (sum_a alpha[a] g(v[b,t,a]) + sum_a beta[a] g(v[b,t-1,a]));   gqd is unchanged.
 * The fold, operation by operation, every operation rounded once (fp32, fused multiply-add where one is written):
 *   C = h(q[b,t]);  L[d] = g(q[b,t])[d];  U[d] = 0
 *   for a = 0 .. n_interp-1, only where the segment t -> t+1 exists:
 *       wa = w_via * alpha[a];  wb = w_via * beta[a]
 *       C = fma(w_via, h(v[b,t,a]), C);  L[d] = fma(wa, g(v[b,t,a])[d], L[d]);  U[d] = fma(wb, g(v[b,t,a])[d], U[d])
 *   gc[b,t][d] = L[b,t][d] + U[b,t-1][d]   (U[b,-1] = 0)
 * after which C and gc take the place of the rollout's cost and gradient in trk_rollout_gp_adam_steps: cost = fma(0.5, prior, C), the
 * gradient of q is gc + the prior's, a pinned component's gradient is zero, Adam as there.  A sample without a segment (t =
 * horizon-1) leaves the sums by a select, not by a zero weight, and the prior's factor of a missing segment is zero by a select: a
 * non-finite trajectory does not reach another trajectory's rows.  At horizon 1 (no segment) gc = g(q) exactly.
 * alpha, beta: DEVICE [n_interp].  Validation (before any device work): everything trk_rollout_gp_adam_steps checks; null via /
 * alpha / beta, n_interp < 1 or a non-finite w_via: TRK_ERR_INVALID_ARG.  TRK_ERR_UNSUPPORTED as there (horizon not a power of two <=
 * TRK_TRAJ_ADAM_MAX_HORIZON; no unit of the model carries k_traj_via_adam; none matches the cost model; generated kernels off).
 * batch = 0: TRK_OK without a launch.  At most 32 iterations per launch, more = several launches inside the call, the result does
 * not depend on the grouping.  trk_last_dispatch: TRK_DISPATCH_GENERATED_VIA_ADAM.  No host synchronisation: capturable. */
typedef struct TrkTrajVia {
    float w_via;                /* finite */
    int32_t n_interp;           /* >= 1 */
    const float* alpha;         /* DEVICE [n_interp] */
    const float* beta;          /* DEVICE [n_interp] */
} TrkTrajVia;
int trk_rollout_gp_via_adam_steps(const TrkModel* model, const TrkCostModel* cm, const TrkRolloutWeights* weights, const TrkGpPrior* gp,
                                  const TrkTrajVia* via, const TrkTrajAdam* adam, float* q, float* qd, float* adam_m, float* adam_v,
                                  int64_t batch, int32_t horizon, float* cost, trk_stream_t stream);

/* trk_rollout_gp_adam_steps for the attached-point models (link spheres, grasped-object points): the planning loop on the objective
 * of trk_rollout_points_cost_grad -- the collision fields on the points of `ps`, the EE term -- plus the constant-velocity GP prior.
 * Buffers, pin, first_step, cost, lr = 0, the 32 iterations per launch and the grouping rule are trk_rollout_gp_adam_steps'.
 * Validation (before any device work), in this order: everything trk_rollout_gp_adam_steps checks except the column count, horizon
 * rule included (TRK_ERR_UNSUPPORTED unless a power of two <= TRK_TRAJ_ADAM_MAX_HORIZON); then the point set as
 * trk_rollout_points_cost_grad checks it (null, of no model or of another model, cost model n_links_in != its points, ee_link):
 * TRK_ERR_INVALID_ARG.  Served by a generated kernel only (k_padam: attached-point units of robots up to 8 DOF, a satellite unit
 * spec_<ident>_padam); TRK_ERR_UNSUPPORTED with the reason when no unit of the point set carries the kernel (a unit loaded as a code
 * object through hipRTC has none), when none bakes the cost model's column sets, or when trk_model_enable_specialized is off.
 * batch = 0: TRK_OK without a launch.  trk_last_dispatch: TRK_DISPATCH_GENERATED.  No host synchronisation: capturable. */
int trk_rollout_points_gp_adam_steps(const TrkModel* model, const TrkPointSet* ps, const TrkCostModel* cm,
                                     const TrkRolloutWeights* weights, const TrkGpPrior* gp, const TrkTrajAdam* adam, float* q, float* qd,
                                     float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost, trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * 3-D point mass (RobotPointMass3D in EnvSpheres3D, EnvTableShelf, EnvMazeBoxes3D or a voxel grid): the trajectory objective and the
 * planning loop, the 3-D siblings of trk_scene2d_traj_via_cost_grad / trk_scene2d_traj_via_adam_steps.  The sample IS the collision
 * point, so there is no TrkModel: `cm` is a cost model with exactly one position column (n_links_in = 1, one object-collision column,
 * no virtual columns), as PlanningTask builds it for the robot.  BUILD-DEFINED like the prior.
 *   q, qd [batch, horizon, 3] fp32, the samples of a trajectory consecutive; adam_m, adam_v [batch, horizon, 6] = [q part | qd part]
 *   per sample; everything contiguous and 4-byte aligned.  1 <= horizon <= TRK_POINT3D_MAX_HORIZON (one lane per sample, a workgroup
 *   of 256 lanes owns whole trajectories): TRK_ERR_UNSUPPORTED above.
 * With h, g the hinge at a point and its gradient -- w_obj * (objects) + w_ws * (workspace box) at the margin of the column, each
 * under the cost model's clamp_fields, the arithmetic of trk_cost_fields (bit for bit at w_obj = w_ws = 1; a zero weight skips the
 * term; w_self and w_ee must be zero where the cost model has self pairs / a tracked link) -- the objective of sample t is
 *   C = h(q[b,t]);  L[d] = g(q[b,t])[d];  U[d] = 0                 and, with a via term, TrkTrajVia's fold (above) on the segment t -> t+1:
 *       C = fma(w_via, h(v[b,t,a]), C);  L[d] = fma(w_via * alpha[a], g(v[b,t,a])[d], L[d]);  U[d] = fma(w_via * beta[a], g(v[b,t,a])[d], U[d])
 *       in ascending a, v[b,t,a] = q[b,t] * alpha[a] + q[b,t+1] * beta[a] with each product and the sum rounded once;
 *   cost[b,t] = fma(gp.weight, P[b,t], C),   P[b,t] = 1/2 e_t^T Q^-1 e_t summed over the coordinates, the factor t -> t+1 attributed
 *       to sample t and 0 at t = horizon-1 (the expressions of trk_scene2d_traj_cost_grad's prior);
 *   gq[b,t]   = (L[b,t] + U[b,t-1]) + gp.weight * d P / d q[b,t]   (U[b,-1] = 0; without a via term just L),
 *   gqd[b,t]  = gp.weight * d P / d qd[b,t].
 * A sample without a segment or without a predecessor leaves the sums by a select, never by a zero weight: a non-finite trajectory
 * does not reach another trajectory's rows.  via = NULL: no via term (then cost and gq are the plain objective's).
 * trk_point3d_traj_cost_grad: one evaluation.  cost [batch, horizon]; gq, gqd [batch, horizon, 3] nullable TOGETHER (cost only).
 * trk_point3d_traj_adam_steps: n_steps iterations of Adam on that objective with (q, qd, m, v) of a sample in its lane's registers,
 * read once and written once per launch -- the arithmetic, the bias terms (formed in double on the host), pin, first_step and the
 * 32 iterations per launch of trk_scene2d_traj_adam_steps; more iterations = several launches inside the call, and the result does
 * not depend on how iterations are grouped into launches or calls.  cost (nullable) [batch, horizon]: the objective of the state as
 * passed in.  lr = 0 (or n_steps = 0) only evaluates: nothing but cost is written.
 * Validation, before any device work (also with batch = 0).  TRK_ERR_INVALID_ARG: null cm / weights / prior / adam, null buffers
 * (batch > 0), non-finite weights, dt, sigma (or dt, sigma <= 0), lr or w_via, pin outside 0 .. 15, first_step < 1, n_steps < 0, a
 * via with null alpha / beta or n_interp < 1, only one of gq / gqd.  TRK_ERR_UNSUPPORTED, with the reason: horizon above
 * TRK_POINT3D_MAX_HORIZON (trk_cost_fields + trk_gp_prior_cost_grad serve any horizon); a cost model whose columns are not exactly
 * one point; self pairs with w_self != 0 or a tracked link with w_ee != 0.  batch = 0: TRK_OK without a launch.
 * No atomics, no host synchronisation: capturable.  TRK_POINT3D_LDS64=1 in the environment (read per call) sends horizon 64 -- a
 * wavefront is a trajectory there and neighbours in time come by DPP shifts -- through the LDS exchange of the other horizons: the
 * same arithmetic, for comparing the two.
 * --------------------------------------------------------------------------------- */
#define TRK_POINT3D_MAX_HORIZON 256
int trk_point3d_traj_cost_grad(const TrkCostModel* cm, const TrkRolloutWeights* w, const TrkGpPrior* gp,
                               const TrkTrajVia* via /* NULL: no via term */, const float* q, const float* qd,
                               int64_t batch, int32_t horizon, float* cost, float* gq, float* gqd, trk_stream_t stream);
int trk_point3d_traj_adam_steps(const TrkCostModel* cm, const TrkRolloutWeights* w, const TrkGpPrior* gp,
                                const TrkTrajVia* via /* NULL: no via term */, const TrkTrajAdam* adam, float* q, float* qd,
                                float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost, trk_stream_t stream);

/* Which exchange the CALLING THREAD's latest launch of the two entries above used for the neighbours in time: the DPP wavefront shifts
 * (horizon 64) or the LDS exchange (every other horizon, and horizon 64 under TRK_POINT3D_LDS64=1); NONE before the first launch (a
 * call that returned without one -- a refusal, batch = 0 -- leaves the answer as it was).  Both compute the same bits. */
enum { TRK_POINT3D_FORM_NONE = 0, TRK_POINT3D_FORM_DPP = 1, TRK_POINT3D_FORM_LDS = 2 };
int trk_point3d_last_form(void);

/* ---------------------------------------------------------------------------------
 * Multi-particle planning: GP-prior sampling and best-particle pick.  What goes INTO the planning loops above (several particles per
 * problem, drawn from the prior the loops carry as a cost) and what comes OUT of them (one winner per problem).  BUILD-DEFINED like
 * the prior: the reference has no sampler, the arithmetic is specified below and checked against an fp64 restatement.
 *
 * trk_gp_prior_sample: n_particles trajectories per problem from the constant-velocity GP prior of trk_gp_prior_cost_grad,
 * conditioned on the problem's start and goal, in ONE launch.  The noise is an input -- eps, unit normals made by the caller -- so
 * the call is a pure function of its arguments; nothing is drawn inside.
 *   start, goal [n_problems, dof]; start_vel, goal_vel [n_problems, dof], required iff pin_vel and ignored otherwise;
 *   eps [n_problems * n_particles, horizon - 1, dof, 2]; q_min, q_max [dof], nullable TOGETHER; q, qd [n_problems * n_particles,
 *   horizon, dof], particle k of problem p is row p * n_particles + k.  All fp32, contiguous, 4-byte aligned.
 * Per trajectory j and coordinate d, independent of every other (j, d); T = horizon - 1, theta = T dt, s = t / T:
 *   noise   w^p_t = l00 e0,  w^v_t = l10 e0 + l11 e1,  (e0, e1) = eps[j, t, d, :],  l00 = sigma dt^1.5 / sqrt(3),
 *           l10 = sigma (sqrt(3) / 2) sqrt(dt),  l11 = sigma sqrt(dt) / 2: the Cholesky factor of Q = sigma^2 [[dt^3/3, dt^2/2],
 *           [dt^2/2, dt]], formed in double on the host and rounded once (like theta);
 *   walk    p_0 = start, v_0 = pin_vel ? start_vel : 0;  p_{t+1} = p_t + dt v_t + w^p_t,  v_{t+1} = v_t + w^v_t;
 *   pin_vel = 1, r_p = goal - p_T, r_v = goal_vel - v_T (the cubic Hermite weights):
 *           q_t = p_t + (3 s^2 - 2 s^3) r_p + theta (s^3 - s^2) r_v,   qd_t = v_t + ((6 s - 6 s^2) / theta) r_p + (3 s^2 - 2 s) r_v;
 *   pin_vel = 0, v* = (goal - p_T) / theta:   q_t = p_t + t dt v*,   qd_t = v_t + v*.
 * Both are exact draws of the Gaussian  exp(-sum_t 1/2 e_t^T Q^-1 e_t)  of trk_gp_prior_cost_grad given the pinned components (the
 * loops' pin mask 15 and 3); at eps = 0, pin_vel = 0 gives the straight line at constant velocity.
 * The two sums along t are scans across the lanes of the trajectory's workgroup with an association that depends on t alone: a
 * trajectory's bits depend only on its own inputs -- not on its place in the batch, on n_particles, or on how a batch is split into
 * calls -- and a non-finite eps row stays in its trajectory.  Any association of the sums is within (2 horizon + 16) 2^-24 of the
 * same expressions with every term replaced by its absolute value.
 * Endpoints by select: q[j, 0] and q[j, T] are the bits of start and goal; with pin_vel, qd[j, 0] and qd[j, T] those of the
 * velocities.  With limits, the way points 0 < t < T are clamped to [q_min[d], q_max[d]] after conditioning by comparisons (a NaN
 * stays a NaN); endpoints and qd are not touched.
 * 2 <= horizon <= TRK_GP_SAMPLE_MAX_HORIZON (a workgroup owns floor(256 / horizon) whole trajectories),
 * 1 <= dof <= TRK_GP_SAMPLE_MAX_DOF.
 * Validation, before any device work (also with n_problems = 0).  TRK_ERR_INVALID_ARG: null s; dt or sigma non-finite or <= 0;
 * n_particles < 1; pin_vel outside {0, 1}; n_problems < 0, horizon < 2, dof < 1; n_problems * n_particles > 0x3fffffff; null start,
 * goal, eps, q or qd (n_problems > 0); pin_vel with a null velocity; only one of q_min / q_max.  TRK_ERR_UNSUPPORTED, the limit
 * named: horizon above TRK_GP_SAMPLE_MAX_HORIZON, dof above TRK_GP_SAMPLE_MAX_DOF.  n_problems = 0: TRK_OK without a launch.
 * No atomics, no host synchronisation: capturable.
 *
 * trk_traj_select_best: per problem, the particle with the smallest score among the candidates.  A particle is a candidate iff
 * is_free is NULL or non-zero there and its score is not NaN (+-inf are candidates).  Smallest by <; among equal scores (-0.0 equals
 * 0.0) the smallest k.  score [n_problems * n_particles]; is_free [n_problems * n_particles] bytes, NULL = all free;
 * best [n_problems] = the winner's row p * n_particles + k, -1 without a candidate; best_score (nullable) its score, +inf without
 * one; n_free (nullable) the number of non-zero flags, whatever the scores (n_particles with is_free = NULL).  Any n_particles >= 1;
 * the result does not depend on how problems are batched.  TRK_ERR_INVALID_ARG: n_problems < 0, n_particles < 1, their product above
 * 0x3fffffff, null score or best (n_problems > 0).  n_problems = 0: TRK_OK without a launch.  One launch, no atomics: capturable.
 * --------------------------------------------------------------------------------- */
#define TRK_GP_SAMPLE_MAX_HORIZON 256
#define TRK_GP_SAMPLE_MAX_DOF 32
typedef struct TrkGpSample { float dt, sigma; int32_t n_particles; int32_t pin_vel; } TrkGpSample;
int trk_gp_prior_sample(const TrkGpSample* s, const float* start, const float* goal, const float* start_vel, const float* goal_vel,
                        const float* eps, const float* q_min, const float* q_max, int64_t n_problems, int32_t horizon, int32_t dof,
                        float* q, float* qd, trk_stream_t stream);
int trk_traj_select_best(const float* score, const uint8_t* is_free /* NULL: all free */, int64_t n_problems, int32_t n_particles,
                         int64_t* best, float* best_score /* nullable */, int32_t* n_free /* nullable */, trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Trajectory post-processing: spline resampling and way-point variance.  What happens to trajectories AFTER the loops and the pick: a
 * coarse path becomes the dense (q, qd) a loop or a controller takes, and a set of particles gets its diversity metric.
 *
 * trk_traj_spline_resample (reference: smoothen_trajectory trajectory/utils.py:8-34, there one trajectory at a time on the host
 * through scipy): the clamped cubic interpolating spline through every column of y, resampled to n_out positions and velocities, in
 * ONE launch.  y [n_traj, n_points, dim]; pos, vel [n_traj, n_out, dim]; fp32, contiguous, 4-byte aligned; vel may be NULL with
 * vel_mode 0.  Per (trajectory, coordinate) column, independent of every other; N = n_points, S = n_out, h = 1 / (N - 1):
 *   spline  the complete cubic spline through y_0 .. y_{N-1} at the uniform knots i h with zero end slopes -- unique, and scipy's
 *           make_interp_spline(linspace(0, 1, N), y, k=3, bc_type='clamped');
 *   slopes  s_0 = s_{N-1} = 0;  s_{i-1} + 4 s_i + s_{i+1} = 3 (N - 1) (y_{i+1} - y_{i-1}) for 0 < i < N - 1, by the Thomas recurrence
 *           down and up the column:  m_1 = 1/4, m_i = 1 / (4 - m_{i-1}) (formed in double, rounded once; they depend on i alone),
 *           g_i = (3 (N - 1) (y_{i+1} - y_{i-1}) - g_{i-1}) m_i with g_0 = 0,  s_i = g_i - m_i s_{i+1}.  A column is solved
 *           sequentially by one lane: its bits depend only on its own inputs, not on its place in the batch or on how a batch is split;
 *   sample  k of S from integers, never a float comparison: a = k (N - 1), i = a / (S - 1), r = a % (S - 1), tau = r / (S - 1); the
 *           last sample is i = N - 2, tau = 1;
 *   pos     (y_i + (tau^2 (3 - 2 tau)) (y_{i+1} - y_i)) + ((h tau) (1 - tau)) ((1 - tau) s_i - tau s_{i+1}), without contraction.  A
 *           constant column comes back bit-exact; at r = 0 the result is the bits of y_i by select, so the endpoints always equal
 *           the input and, when (S - 1) % (N - 1) == 0, every knot does;
 *   vel     vel_mode 0: zeros.  1: the reference's set_average_velocity as it is: rows 1 .. S-2 are (y_1 - y_0) / (S dt), the two
 *           end rows 0; S dt is formed in double and rounded once.  2: the spline's derivative with respect to its parameter u in
 *           [0, 1] (not time; what the reference returns):  (((6 (N - 1) tau) (1 - tau)) (y_{i+1} - y_i) + ((1 - tau) (1 - 3 tau)) s_i)
 *           + (tau (3 tau - 2)) s_{i+1};  the two end rows are exactly 0 by select.
 * A non-finite value poisons its own column and nothing else.
 * 2 <= n_points <= TRK_SPLINE_MAX_POINTS, 2 <= n_out <= TRK_SPLINE_MAX_OUT, 1 <= dim <= TRK_SPLINE_MAX_DIM.
 * Validation, before any device work (also with n_traj = 0).  TRK_ERR_INVALID_ARG: n_traj < 0, n_points < 2, n_out < 2, dim < 1;
 * n_traj * max(n_points, n_out) > 0x3fffffff; vel_mode outside {0, 1, 2}; vel_mode 1 with dt non-finite or <= 0; vel_mode != 0 with
 * a null vel; null y or pos (n_traj > 0).  TRK_ERR_UNSUPPORTED, the limit named: a value above its maximum.  n_traj = 0: TRK_OK
 * without a launch.  No atomics, no host synchronisation: capturable.
 *
 * trk_traj_waypoint_variance (reference: compute_variance_waypoints trajectory/metrics.py:14-24, there for one set of trajectories):
 * per problem p, the sum over the way points of the variance of the particles' pairwise distances.  x [n_problems * n_particles,
 * horizon, state_dim], particle k of problem p is row p * n_particles + k; the positions are columns c0 .. c0 + dim - 1 (as in
 * trk_traj_diff_norm_sum); out [n_problems].  With K = n_particles and n = K^2 (the reference takes the unbiased variance over the
 * whole triu matrix, zeros included), per way point t:
 *   S1 = sum_{i<j} d_ij,  S2 = sum_{i<j} d_ij^2,  var_t = (S2 - S1^2 / n) / (n - 1),  out[p] = sum_t var_t.
 * d_ij is the Euclidean distance, formed in fp32 from the coordinate differences (sum in ascending coordinate, then the square
 * root) -- not by |a|^2 + |b|^2 - 2 a.b, which loses clustered particles.  S1, S2, the subtraction, the division and the sum over t
 * are fp64, rounded once to fp32.  K = 1 gives NaN like the reference (0 / 0); a non-finite input stays in its own problem.
 * Two launches, no atomics: the particles are cut into tiles of 64, a wavefront sums one (way point, tile pair) and stores its two
 * fp64 sums in the workspace, and the second kernel adds a way point's tile pairs in ascending order, the way points of a lane in
 * ascending order, and the lanes by a fixed tree.  The result is bit-reproducible and does not depend on how problems are batched.
 * workspace: trk_traj_waypoint_variance_workspace_bytes(n_problems, n_particles, horizon) bytes (host-only query; -1 for arguments
 * the entry refuses), 8-byte aligned, the caller's; nothing in it needs zeroing.
 * 1 <= n_particles <= TRK_WAYPOINT_VAR_MAX_PARTICLES, horizon >= 1, 1 <= dim <= TRK_WAYPOINT_VAR_MAX_DIM.
 * Validation, before any device work (also with n_problems = 0).  TRK_ERR_INVALID_ARG: n_problems < 0, n_particles < 1, horizon < 1;
 * n_problems * n_particles * horizon > 0x3fffffff; dim < 1, c0 < 0, c0 + dim > state_dim; null x or out (n_problems > 0).
 * TRK_ERR_UNSUPPORTED, the limit named: n_particles or dim above its maximum.  Then TRK_ERR_INVALID_ARG for a workspace that is
 * null, misaligned or too small (n_problems > 0).  n_problems = 0: TRK_OK without a launch.  Capturable.
 * --------------------------------------------------------------------------------- */
#define TRK_SPLINE_MAX_POINTS 256
#define TRK_SPLINE_MAX_OUT 1024
#define TRK_SPLINE_MAX_DIM 32
#define TRK_WAYPOINT_VAR_MAX_PARTICLES 4096
#define TRK_WAYPOINT_VAR_MAX_DIM 32
int trk_traj_spline_resample(const float* y, int64_t n_traj, int32_t n_points, int32_t dim, int32_t n_out, int32_t vel_mode, float dt,
                             float* pos, float* vel /* nullable */, trk_stream_t stream);
int64_t trk_traj_waypoint_variance_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon);
int trk_traj_waypoint_variance(const float* x, int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t state_dim, int32_t c0,
                               int32_t dim, float* out /* [n_problems] */, void* workspace, int64_t workspace_bytes,
                               trk_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Sampling-based trajectory update: soft-min weights and the weighted particle mean.  The optimiser of STOMP / MPPI for every robot
 * and horizon a cost can be evaluated at: perturb the mean with smooth noise (trk_gp_prior_sample with zero start and goal), evaluate
 * every particle, weight the particles by a soft-min of their costs, move the mean to the weighted particle mean.  These two entries
 * are the last two steps.  BUILD-DEFINED like the sampler: the arithmetic is specified below and checked against restatements.
 * Particle k of problem p is row p * n_particles + k everywhere; K = n_particles, H = horizon.  fp32, contiguous, 4-byte aligned.
 *
 * trk_traj_softmin_weights: cost [n_problems * K, H] (H = 1: the scores are already summed); valid [n_problems * K] bytes, NULL =
 * all valid, 0 = rejected; lambda = s->temperature.  Everything between reading cost and the final rounding is fp64.
 *   TRK_SOFTMIN_TRAJECTORY (MPPI), w [n_problems * K], ess (nullable) [n_problems]:
 *     S_k = sum_t cost[k, t];  a particle is a candidate iff it is valid and S_k is finite;  m = min over the candidates;
 *     a_k = exp(-(S_k - m) / lambda),  Z = sum_k a_k over the candidates;
 *     w_k = (float)(a_k / Z), exactly 0 for a non-candidate;  ess = (float)(Z^2 / sum_k a_k^2).
 *   TRK_SOFTMIN_WAYPOINT (STOMP's probabilities), w [n_problems * K, H], ess (nullable) [n_problems, H], per way point t:
 *     the candidates are the valid particles with finite cost[k, t];  lo, hi their min and max;
 *     a_k = hi > lo ? exp(-(cost[k, t] - lo) / ((hi - lo) lambda)) : 1;  Z, w_k and ess as above.  STOMP's h = 10 is lambda = 0.1.
 *   A problem (or way point) without a candidate gets all weights 0 and ess 0.
 * The association is fixed and a function of H and K alone, so a problem's bits do not depend on its place in the batch or on how
 * the batch is split into calls.  S_k: with G = the power of two >= min(H, 64), G partial sums s_j = cost[k, j] + cost[k, j + G] +
 * ... in ascending t, folded by the xor tree j ^ G/2, .., j ^ 1.  Z and sum a^2: one workgroup of 1024 lanes owns a problem (way-point
 * mode: 16 consecutive way points of it, NG = 64 lanes a way point; trajectory mode NG = 1024); lane g adds the candidates k = g,
 * g + NG, ... in ascending k, and the NG sums fold by the tree sum[g] += sum[g + m] for g < m, m = NG/2, .., 1.  One launch; the trajectory mode with
 * K > 256 and H > 1 takes two: S_k of all rows is formed across the chip first (the same arithmetic, the same bits) and passes
 * through the workspace, so one problem with thousands of particles is not summed by a single workgroup.
 * workspace: trk_traj_softmin_weights_workspace_bytes(n_problems, K, H, mode) bytes (host-only query; 0 where one launch serves,
 * and workspace may then be NULL; -1 for arguments the entry refuses), 8-byte aligned, the caller's; nothing in it needs zeroing.
 *
 * trk_traj_weighted_update: out = mean + step * sum_k w_k (x_k - mean).  x [n_problems * K, H, dim]; mean, out [n_problems, H, dim]
 * (out == mean is allowed); w [n_problems * K], or [n_problems * K, H] with w_per_waypoint = 1; lo, hi [dim], nullable TOGETHER.
 * Per element, in fp32, every operation rounded once (no contraction):  d = x_k - mean,  acc = acc + w_k * d,  out = mean + step * acc.
 *   A particle whose weight is exactly 0 (+-0) leaves the sum by a select, not by its zero product: a NaN row of a rejected particle
 *   does not reach the mean.
 *   Order of the K terms: chunks of 64 particles (the last one shorter); a chunk's sum starts from +0 and adds its terms in ascending
 *   k; the result is chunk 0's sum, then + chunk 1's, .. in ascending chunk order.  A function of k and K alone: a problem's bits
 *   do not depend on the batch.
 *   step = 0: mean + step * acc is replaced by mean's bits by select.
 *   pin: bit 0 keeps the first way point, bit 1 the last -- the output is mean's bits by select, whatever the limits say.
 *   With limits the unpinned result r is clamped by comparisons, r < lo[d] ? lo[d] : r, then r > hi[d] ? hi[d] : r: a NaN stays a NaN.
 * x is read exactly once; a wavefront's loads cover 64 consecutive floats of a particle's H * dim row.  K <= 64: one launch, a
 * wavefront per (problem, 64 elements).  K > 64: a wavefront per (problem, chunk, 64 elements) stores the chunk's sum in the
 * workspace [n_problems, ceil(K / 64), H * dim] fp32, and a second launch adds the chunks and finishes: one problem with thousands of
 * particles fills the chip as many problems with few do.
 * workspace: trk_traj_weighted_update_workspace_bytes(n_problems, K, H, dim) bytes (host-only query; 0 for K <= 64, where workspace
 * may be NULL; -1 for arguments the entry refuses), 4-byte aligned, the caller's; nothing in it needs zeroing.
 * Any association of the K terms is within (K + 3) 2^-24 of  |mean| + |step| sum_k |w_k| |x_k - mean|  (each term's difference,
 * product and addition, then the step and the final addition).
 *
 * 1 <= n_particles <= TRK_SOFTMIN_MAX_PARTICLES, horizon >= 1, dim >= 1.
 * Validation, before any device work (also with n_problems = 0).  TRK_ERR_INVALID_ARG: a null struct; temperature non-finite or
 * <= 0; step non-finite; mode outside {0, 1}, pin outside 0 .. 3, w_per_waypoint outside {0, 1}; n_problems < 0, n_particles < 1,
 * horizon < 1, dim < 1; n_problems * n_particles or horizon * dim above 0x3fffffff, more than 0x7fffffff workgroups; only one of
 * lo / hi; null cost, w, x, mean or out (n_problems > 0).  TRK_ERR_UNSUPPORTED, the limit named: n_particles above the maximum.  Then
 * TRK_ERR_INVALID_ARG for a workspace that is null, misaligned or too small (n_problems > 0 and the query above 0).  n_problems = 0: TRK_OK
 * without a launch.  No atomics, no host synchronisation: capturable.
 * --------------------------------------------------------------------------------- */
#define TRK_SOFTMIN_MAX_PARTICLES 4096
enum { TRK_SOFTMIN_TRAJECTORY = 0, TRK_SOFTMIN_WAYPOINT = 1 };
typedef struct TrkSoftmin { float temperature; int32_t mode; int32_t n_particles; } TrkSoftmin;
typedef struct TrkWeightedUpdate { float step; int32_t pin; int32_t n_particles; int32_t w_per_waypoint; } TrkWeightedUpdate;
int trk_traj_softmin_weights(const TrkSoftmin* s, const float* cost, const uint8_t* valid /* NULL: all valid */, int64_t n_problems,
                             int32_t horizon, float* w, float* ess /* nullable */, void* workspace, int64_t workspace_bytes,
                             trk_stream_t stream);
int64_t trk_traj_softmin_weights_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t mode);
int64_t trk_traj_weighted_update_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t dim);
int trk_traj_weighted_update(const TrkWeightedUpdate* u, const float* x, const float* mean, const float* w, const float* lo,
                             const float* hi, int64_t n_problems, int32_t horizon, int32_t dim, float* out, void* workspace,
                             int64_t workspace_bytes, trk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TRK_H */

// trk_point3d.hip -- the 3-D point mass (include/trk.h, "3-D point mass"): RobotPointMass3D + PlanningTask on the reference's 3-D scenes
// (EnvSpheres3D, EnvTableShelf, EnvMazeBoxes3D, a voxel grid).  A sample is one point and that point is the cost model's only column,
// so the kernel is one lane per sample like trk_planar.hip's traj_loop, with the scene walk of the table-driven field kernels
// (scene_min_sdf<1>, ws_cost_point: trk_device.h) in place of the planar scene.
#include <hip/hip_runtime.h>
#include "trk_launch.h"

namespace {

// The hinge of one point, cost and gradient: what fields_links<1> (trk_kernels.hip) computes for a cost model with one column, the same
// operations in the same order -- scene_min_sdf<1>, the clamp_fields select, ws_cost_point -- and the `0 +` with which k_cost_fields
// folds a column into its sums.  At w_obj = w_ws = 1 the results are trk_cost_fields' own bits.  A zero weight skips the term.
__device__ __forceinline__ float point_hinge(const DevCostHdr& C, float w_obj, float w_ws, float mg, float x, float y, float z,
                                             float& gx_out, float& gy_out, float& gz_out) {
    const float px[1] = {x}, py[1] = {y}, pz[1] = {z};
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    float cost = 0.0f;
    if (w_obj != 0.0f && C.n_objects > 0) {
        float s[1], gx[1], gy[1], gz[1];
        scene_min_sdf<1>(C, px, py, pz, s, gx, gy, gz);
        const float v = mg - s[0];
        const bool off = (C.clamp_fields & TRK_FIELD_OBJECTS) && !(v > 0.0f);           // clamp_sdf: relu(margin - sdf)
        const float wk = off ? 0.0f : w_obj;
        cost = fmaf(wk, v, cost);
        ax -= wk * gx[0]; ay -= wk * gy[0]; az -= wk * gz[0];
    }
    if (w_ws != 0.0f && C.has_ws) cost = fmaf(w_ws, ws_cost_point(C, mg, x, y, z, w_ws, ax, ay, az), cost);
    gx_out = 0.0f + ax; gy_out = 0.0f + ay; gz_out = 0.0f + az;
    return 0.0f + cost;
}

// One coordinate of the prior at sample t from its neighbours: gp_coord of trk_planar.hip (k_gp_prior's element()), the same
// operations in the same order.  acc gathers the factor t -> t+1 (attributed to t); gp, gv are d prior / d q[t], d prior / d qd[t].
__device__ __forceinline__ void gp_coord(const Point3DPar& P, bool has_prev, bool has_next, float p0, float v0, float pm, float vm,
                                         float pn, float vn, float& acc, float& gp, float& gv) {
    gp = 0.0f; gv = 0.0f;
    if (has_next) {
        const float ep = fmaf(P.dt, v0, p0) - pn, ev = v0 - vn;
        const float rp = fmaf(P.a, ep, P.b * ev), rv = fmaf(P.b, ep, P.c * ev);
        acc = fmaf(0.5f, fmaf(ep, rp, ev * rv), acc);
        gp = rp; gv = fmaf(P.dt, rp, rv);
    }
    if (has_prev) {
        const float ep = fmaf(P.dt, vm, pm) - p0, ev = vm - v0;
        gp -= fmaf(P.a, ep, P.b * ev); gv -= fmaf(P.b, ep, P.c * ev);
    }
    gp *= P.w; gv *= P.w;
}

// adam_component of trk_planar.hip (trk_ik_step's Adam on one component), every operation rounded once
__device__ __forceinline__ void adam_component(float g, float step, float rsqrt_bc2, float& x, float& m, float& v) {
    const float m1 = fmaf(0.9f, m, 0.1f * g);
    const float v1 = fmaf(0.999f, v, 0.001f * g * g);
    m = m1; v = v1;
    const float denom = fmaf(sqrtf(v1), rsqrt_bc2, 1e-8f);
    x = x - step * (m1 / denom);
}

// The persistent loop of both entries (trk_point3d_traj_cost_grad: update == 0, one iteration, which also stores the gradient;
// trk_point3d_traj_adam_steps), the 3-D sibling of traj_loop in trk_planar.hip.
// One lane per sample, a workgroup of 256 lanes owns floor(256 / H) whole trajectories (lanes beyond them idle); x = (q, qd) of a
// sample and Adam's m, v (6 floats each) stay in its lane's registers for the n_steps iterations of the launch: read once, written
// once.  Each iteration a lane needs x of t - 1 and t + 1:
//   WAVE (H == 64, a wavefront is a trajectory): two DPP wavefront shifts per value, no LDS and no barrier;
//   otherwise: through LDS (component-major: lane tid reads word tid +- 1 of a row, no bank conflict), two buffers used in turn and
//   ONE barrier per iteration -- a lane that writes buffer k & 1 for iteration k + 2 has passed the barrier of iteration k + 1, which
//   every lane reaches only after its reads of iteration k.
// VIA: TrkTrajVia's fold.  After the first exchange a lane with a segment (t < H - 1) walks the segment's n via points with (C, L, U)
// in registers, and U goes to lane t + 1:
//   WAVE: three more DPP shifts;
//   otherwise: three floats per lane through LDS, ONE buffer and a second barrier per iteration.  A lane that writes uch for iteration
//   k + 1 has passed the first barrier of iteration k + 1, which every lane reaches only after its read of uch in iteration k; a lane
//   that reads uch in iteration k has passed the second barrier of iteration k, which every lane reaches only after its write.
// Idle lanes (beyond the workgroup's whole trajectories, or beyond the batch) reach every barrier; n_steps is uniform for the launch.
// Only a whole inactive wavefront of the WAVE form returns early.  The lane without a segment and the lane without a predecessor have
// their shares removed by a select: what lane tid - 1 of another trajectory wrote never enters.
// The structs come by value: the fields stay scalar loads from the kernarg segment, the scene tables scalar loads through cptr().
template <bool WAVE, bool VIA>
__global__ void __launch_bounds__(256)
k_point3d_traj(const DevCostHdr C, const Point3DPar P, float* __restrict__ q, float* __restrict__ qd, float* __restrict__ mom,
               float* __restrict__ vel, int64_t B, int H, float* __restrict__ cost, float* __restrict__ gq, float* __restrict__ gqd) {
    __shared__ float xch[WAVE ? 1 : 2][WAVE ? 1 : 6][WAVE ? 1 : 256];
    __shared__ float uch[WAVE || !VIA ? 1 : 3][WAVE || !VIA ? 1 : 256];
    const int tid = threadIdx.x;
    const int per_wg = WAVE ? 4 : 256 / H;
    const int tl = WAVE ? tid >> 6 : tid / H;                      // the lane's trajectory within the workgroup
    const int t = WAVE ? tid & 63 : tid - tl * H;
    const int64_t traj = (int64_t)blockIdx.x * per_wg + tl;
    const bool active = tl < per_wg && traj < B;
    if (WAVE && !active) return;                                   // a whole wavefront: the DPP shifts below see all 64 lanes
    const int64_t s = traj * H + t;
    const bool has_prev = t > 0, has_next = t + 1 < H;
    const bool update = P.update != 0;
    float x[6], m[6], v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { x[k] = 0.0f; m[k] = 0.0f; v[k] = 0.0f; }
    if (active) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { x[k] = q[3 * s + k]; x[3 + k] = qd[3 * s + k]; }
        if (update) {
#pragma unroll
            for (int k = 0; k < 6; ++k) { m[k] = mom[6 * s + k]; v[k] = vel[6 * s + k]; }
        }
    }
    const float mg = cptr(C.obj_link_margin)[0];
    // a pinned component's gradient is taken as zero
    const bool pin_q = ((P.pin & 1) && t == 0) || ((P.pin & 2) && t == H - 1);
    const bool pin_qd = ((P.pin & 4) && t == 0) || ((P.pin & 8) && t == H - 1);
    for (int it = 0; it < P.n_steps; ++it) {
        float xm[6], xn[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { xm[k] = x[k]; xn[k] = x[k]; }
        if constexpr (WAVE) {
#pragma unroll
            for (int k = 0; k < 6; ++k) { xm[k] = trk_dpp_from_prev(x[k], x[k]); xn[k] = trk_dpp_from_next(x[k], x[k]); }
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) xch[it & 1][k][tid] = x[k];
            __syncthreads();
            if (active && has_prev) {
#pragma unroll
                for (int k = 0; k < 6; ++k) xm[k] = xch[it & 1][k][tid - 1];
            }
            if (active && has_next) {
#pragma unroll
                for (int k = 0; k < 6; ++k) xn[k] = xch[it & 1][k][tid + 1];
            }
        }
        // C, L, U of TrkTrajVia's fold; without a via term just the hinge at the sample
        float c = 0.0f, l[3] = {0.0f, 0.0f, 0.0f}, u[3] = {0.0f, 0.0f, 0.0f};
        if (active) c = point_hinge(C, P.w_obj, P.w_ws, mg, x[0], x[1], x[2], l[0], l[1], l[2]);
        if constexpr (VIA) {
            if (active && has_next) {
                const TRK_CAS float* al = cptr(P.alpha);
                const TRK_CAS float* be = cptr(P.beta);
#pragma nounroll
                for (int a = 0; a < P.via_n; ++a) {
                    const float fa = al[a], fb = be[a];
                    const float wa = P.w_via * fa, wb = P.w_via * fb;
                    const float vx = __fadd_rn(__fmul_rn(x[0], fa), __fmul_rn(xn[0], fb));
                    const float vy = __fadd_rn(__fmul_rn(x[1], fa), __fmul_rn(xn[1], fb));
                    const float vz = __fadd_rn(__fmul_rn(x[2], fa), __fmul_rn(xn[2], fb));
                    float g0, g1, g2;
                    const float h = point_hinge(C, P.w_obj, P.w_ws, mg, vx, vy, vz, g0, g1, g2);
                    c = fmaf(P.w_via, h, c);
                    l[0] = fmaf(wa, g0, l[0]); l[1] = fmaf(wa, g1, l[1]); l[2] = fmaf(wa, g2, l[2]);
                    u[0] = fmaf(wb, g0, u[0]); u[1] = fmaf(wb, g1, u[1]); u[2] = fmaf(wb, g2, u[2]);
                }
            }
            float up[3] = {0.0f, 0.0f, 0.0f};
            if constexpr (WAVE) {
#pragma unroll
                for (int k = 0; k < 3; ++k) up[k] = trk_dpp_from_prev(0.0f, u[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) uch[k][tid] = u[k];
                __syncthreads();
                if (active && has_prev) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) up[k] = uch[k][tid - 1];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k] = l[k] + (has_prev ? up[k] : 0.0f);       // gc = L + U[t-1], U[-1] = 0
        }
        if (active) {
            float acc = 0.0f, gp[3], gv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) gp_coord(P, has_prev, has_next, x[k], x[3 + k], xm[k], xm[3 + k], xn[k], xn[3 + k], acc, gp[k], gv[k]);
            const float ct = fmaf(P.w, acc, c);
            float g[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) { g[k] = l[k] + gp[k]; g[3 + k] = gv[k]; }
            if (it == 0 && cost) cost[s] = ct;
            if (it == 0 && !update && gq) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { gq[3 * s + k] = g[k]; gqd[3 * s + k] = g[3 + k]; }
            }
            if (update) {
                const float step = P.lr / P.bc1[it], rs = P.rsqrt_bc2[it];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    adam_component(pin_q ? 0.0f : g[k], step, rs, x[k], m[k], v[k]);
                    adam_component(pin_qd ? 0.0f : g[3 + k], step, rs, x[3 + k], m[3 + k], v[3 + k]);
                }
            }
        }
    }
    if (active && update) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[3 * s + k] = x[k]; qd[3 * s + k] = x[3 + k]; }
#pragma unroll
        for (int k = 0; k < 6; ++k) { mom[6 * s + k] = m[k]; vel[6 * s + k] = v[k]; }
    }
}

template <bool WAVE, bool VIA>
void launch(const DevCostHdr& C, const Point3DPar& P, float* q, float* qd, float* m, float* v, int64_t B, int H, float* cost, float* gq,
            float* gqd, hipStream_t st) {
    const int per_wg = WAVE ? 4 : 256 / H;
    const dim3 g((unsigned)((B + per_wg - 1) / per_wg)), b(256);
    hipLaunchKernelGGL((k_point3d_traj<WAVE, VIA>), g, b, 0, st, C, P, q, qd, m, v, B, H, cost, gq, gqd);
}

}  // namespace

void trk_launch_point3d_traj(const DevCostHdr& C, const Point3DPar& P, bool wave, float* q, float* qd, float* adam_m, float* adam_v,
                             int64_t batch, int horizon, float* cost, float* gq, float* gqd, hipStream_t st) {
    const bool via = P.via_n > 0;
    if (wave) {
        if (via) launch<true, true>(C, P, q, qd, adam_m, adam_v, batch, horizon, cost, gq, gqd, st);
        else launch<true, false>(C, P, q, qd, adam_m, adam_v, batch, horizon, cost, gq, gqd, st);
    } else {
        if (via) launch<false, true>(C, P, q, qd, adam_m, adam_v, batch, horizon, cost, gq, gqd, st);
        else launch<false, false>(C, P, q, qd, adam_m, adam_v, batch, horizon, cost, gq, gqd, st);
    }
}

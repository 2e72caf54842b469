// trk_planar.hip -- the 2-D point mass in a planar scene (include/trk.h, "2-D point mass"): RobotPointMass + PlanningTask on the
// reference's 2-D scenes (EnvDense2D, EnvNarrowPassageDense2D, ...).  A sample is one point, so every kernel is one lane per sample:
// q in as one float2, the cost out as one coalesced fp32 store and the gradient as one float2.
//
// The scene is a handful of analytic objects (at most a few dozen primitives) and/or a precomputed 2-D SDF grid.  The analytic
// tables are the same for every lane: the kernels walk them with loop counters through the constant address space, so the compiler
// fetches them with scalar loads into SGPRs.  The grid is packed as float4 (sdf, gx, gy, 0) per cell, so a lookup is ONE 16-byte
// gather; 400 x 400 cells are 2.56 MB and stay in an XCD's 4 MiB L2 across launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include "trk_launch.h"

namespace {

struct alignas(16) P2Prim {     // 8 dwords
    int32_t type;
    float cx, cy, hx, hy, r;
    int32_t _pad[2];
};

struct alignas(16) P2Obj {      // 16 dwords
    float pos[3];
    float R[9];
    int32_t begin, end;
    int32_t kind;               // 0: R = I and pos = 0 (local = q), 1: R = I (local = q - pos), 2: general
    int32_t _pad;
};

// Passed to kernels by value (kernarg segment, scalar-loaded).
struct P2Hdr {
    const P2Obj* objs;          // device [n_objects]
    const P2Prim* prims;        // device
    const float4* cells;        // device [nx * ny] = (sdf, gx, gy, 0), row-major (i, j)
    int32_t n_objects, has_grid, nx, ny;
    float lim0, lim1, md0, md1, fd0, fd1;
    float ws_min0, ws_min1, ws_max0, ws_max1;
    float margin;
};

// sphere primitives.py:108-112, sharp box :220-223, rounded box :327-334 in 2-D, with the gradients torch's autograd gives them:
// norm' = v / |v| (0 at 0), abs' = sign (0 at +-0), max(dim)' to the first maximum, amax' split evenly between equal values,
// minimum(a, 0)' split at a == 0, relu'(0) = 0.
__device__ __forceinline__ float prim2d_sdf(const TRK_CAS P2Prim* P, float x, float y, float& gx, float& gy) {
    const int type = P->type;
    const float dx = x - P->cx, dy = y - P->cy;
    if (type == TRK_PRIM_SPHERE) {
        const float n = sqrtf(dx * dx + dy * dy);
        const float inv = n > 0.0f ? 1.0f / n : 0.0f;
        gx = dx * inv; gy = dy * inv;
        return n - P->r;
    }
    const float sx = dx > 0.0f ? 1.0f : (dx < 0.0f ? -1.0f : 0.0f);
    const float sy = dy > 0.0f ? 1.0f : (dy < 0.0f ? -1.0f : 0.0f);
    if (type == TRK_PRIM_SHARP_BOX) {
        const float ux = fabsf(dx) - P->hx, uy = fabsf(dy) - P->hy;
        const bool ay = uy > ux;                                   // first maximum wins
        gx = ay ? 0.0f : sx; gy = ay ? sy : 0.0f;
        return ay ? uy : ux;
    }
    const float r = P->r;
    const float ux = fabsf(dx) - P->hx + r, uy = fabsf(dy) - P->hy + r;
    const float mu = fmaxf(ux, uy);
    const float wx = ux == uy ? 0.5f : (ux > uy ? 1.0f : 0.0f), wy = 1.0f - wx;       // amax: ties share
    const float inside = mu < 0.0f ? 1.0f : (mu == 0.0f ? 0.5f : 0.0f);               // minimum(max_q, 0)
    const float rx = fmaxf(ux, 0.0f), ry = fmaxf(uy, 0.0f);
    const float nn = sqrtf(rx * rx + ry * ry);
    const float inv = nn > 0.0f ? 1.0f / nn : 0.0f;
    gx = (inside * wx + rx * inv) * sx;
    gy = (inside * wy + ry * inv) * sy;
    return (fminf(mu, 0.0f) + nn) - r;
}

// ObjectField in 2-D (primitives.py:387-405): (x, y, 0) - pos, rotated by R^T, first two coordinates; min over the primitives (first
// minimum wins); the gradient goes back through the upper-left 2 x 2 block of R.
__device__ __forceinline__ float object2d_sdf(const P2Hdr& S, int o, float x, float y, float& gx, float& gy) {
    const TRK_CAS P2Obj* O = cptr(S.objs) + o;
    const int kind = O->kind;
    float lx = x, ly = y;
    if (kind == 1) { lx = x - O->pos[0]; ly = y - O->pos[1]; }
    else if (kind == 2) {
        const float dx = x - O->pos[0], dy = y - O->pos[1], dz = 0.0f - O->pos[2];
        lx = O->R[0] * dx + O->R[3] * dy + O->R[6] * dz;
        ly = O->R[1] * dx + O->R[4] * dy + O->R[7] * dz;
    }
    float best = __builtin_inff(), bx = 0.0f, by = 0.0f;
    const int end = O->end;
    for (int i = O->begin; i < end; ++i) {
        float px, py;
        const float v = prim2d_sdf(cptr(S.prims) + i, lx, ly, px, py);
        const bool take = v < best;
        best = take ? v : best; bx = take ? px : bx; by = take ? py : by;
    }
    if (kind == 2) { gx = O->R[0] * bx + O->R[1] * by; gy = O->R[3] * bx + O->R[4] * by; }
    else { gx = bx; gy = by; }
    return best;
}

// GridMapSDF.get_sdf in 2-D (grid_map_sdf.py:81-114): the nearest-lower cell, clamped; its stored value and gradient
__device__ __forceinline__ float4 grid2d_cell(const P2Hdr& S, float x, float y) {
    const int i = grid_axis_cell(x, S.lim0, S.md0, S.fd0, S.nx);
    const int j = grid_axis_cell(y, S.lim1, S.md1, S.fd1, S.ny);
    return S.cells[(int64_t)i * S.ny + j];
}

// torch.linspace(lo, hi, n)[i]: start + i * step for the first half, end - (n - 1 - i) * step after (the 3-D precompute's rule);
// a single node is the START, torch.linspace(lo, hi, 1) = [lo]
__device__ __forceinline__ float linspace_at(float lo, float hi, int n, int i) {
    if (n == 1) return lo;
    const float step = (hi - lo) / (float)(n - 1);
    return i < n / 2 ? lo + step * (float)i : hi - step * (float)(n - 1 - i);
}

// The object term: max over the df objects of (m - sdf_o), first maximum wins; gradient -grad sdf of that object.
template <bool GRID, bool ANALYTIC>
__device__ __forceinline__ float objects_term(const P2Hdr& S, float m, float x, float y, float& gx, float& gy) {
    float best = -__builtin_inff(), bx = 0.0f, by = 0.0f;
    if (GRID) {
        const float4 c = grid2d_cell(S, x, y);
        best = m - c.x; bx = c.y; by = c.z;
    }
    if (ANALYTIC) {
        for (int o = 0; o < S.n_objects; ++o) {
            float ox, oy;
            const float v = m - object2d_sdf(S, o, x, y, ox, oy);
            const bool take = v > best;
            best = take ? v : best; bx = take ? ox : bx; by = take ? oy : by;
        }
    }
    gx = -bx; gy = -by;
    return best;
}

// CollisionWorkspaceBoundariesDistanceField (distance_fields.py:319-332): faces x - min, y - min, max - x, max - y, each through
// sign(d) |d| (value d, derivative 0 at d == 0); max over the faces of (m - d), first maximum wins.
__device__ __forceinline__ float ws_term(const P2Hdr& S, float m, float x, float y, float& gx, float& gy) {
    const float d0 = x - S.ws_min0, d1 = y - S.ws_min1, d2 = S.ws_max0 - x, d3 = S.ws_max1 - y;
    float best = m - d0; int k = 0;
    if (m - d1 > best) { best = m - d1; k = 1; }
    if (m - d2 > best) { best = m - d2; k = 2; }
    if (m - d3 > best) { best = m - d3; k = 3; }
    const float d = k == 0 ? d0 : (k == 1 ? d1 : (k == 2 ? d2 : d3));
    const float s = d != 0.0f ? 1.0f : 0.0f;
    gx = k == 0 ? -s : (k == 2 ? s : 0.0f);
    gy = k == 1 ? -s : (k == 3 ? s : 0.0f);
    return best;
}

template <bool GRID, bool ANALYTIC, bool WS>
__device__ __forceinline__ bool collides(const P2Hdr& S, float m, float x, float y) {
    bool hit = false;
    if (GRID) hit = grid2d_cell(S, x, y).x < m;
    if (ANALYTIC) {
        for (int o = 0; o < S.n_objects; ++o) {
            float gx, gy;
            hit = hit || object2d_sdf(S, o, x, y, gx, gy) < m;
        }
    }
    if (WS) hit = hit || (x - S.ws_min0) < m || (y - S.ws_min1) < m || (S.ws_max0 - x) < m || (S.ws_max1 - y) < m;
    return hit;
}

// The hinge of one sample, cost and gradient: the body of k_planar_cost, and of the trajectory kernels below -- one function, so
// that all of them run the same instruction sequence on a sample (what the trajectory kernels' tests lean on).
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP>
__device__ __forceinline__ float hinge_term(const P2Hdr& S, float2 p, float& gx_out, float& gy_out) {
    float c = 0.0f, gx = 0.0f, gy = 0.0f;
    if (GRID || ANALYTIC) {
        float ox, oy;
        const float v = objects_term<GRID, ANALYTIC>(S, S.margin, p.x, p.y, ox, oy);
        const bool live = !CLAMP || v > 0.0f;                      // relu: no gradient at or below zero
        c = CLAMP ? fmaxf(v, 0.0f) : v;
        gx = live ? ox : 0.0f; gy = live ? oy : 0.0f;
    }
    if (WS) {
        float wx, wy;
        const float v = ws_term(S, S.margin, p.x, p.y, wx, wy);
        const bool live = !CLAMP || v > 0.0f;
        c = c + (CLAMP ? fmaxf(v, 0.0f) : v);
        gx = gx + (live ? wx : 0.0f); gy = gy + (live ? wy : 0.0f);
    }
    gx_out = gx; gy_out = gy;
    return c;
}

template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP, bool GRAD>
__global__ void __launch_bounds__(256)
k_planar_cost(P2Hdr S, const float2* __restrict__ q, int64_t n, float* __restrict__ cost, float2* __restrict__ grad) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    float gx, gy;
    cost[s] = hinge_term<GRID, ANALYTIC, WS, CLAMP>(S, q[s], gx, gy);
    if (GRAD) grad[s] = make_float2(gx, gy);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The trajectory objective: w_obj x the hinge + the constant-velocity GP prior on (q, qd), one lane per sample (include/trk.h).
// ---------------------------------------------------------------------------------------------------------------------------
struct TrajPar { float w_obj, dt, a, b, c, w; };        // a, b, c: the entries of Q^-1 as trk_launch_gp_prior forms them

// One coordinate of the prior at sample t from its neighbours: k_gp_prior's element(), the same operations in the same order.
// acc gathers the factor t -> t+1 (attributed to t); gp, gv are d prior / d q[t], d prior / d qd[t].
__device__ __forceinline__ void gp_coord(const TrajPar& P, bool has_prev, bool has_next, float p0, float v0, float pm, float vm,
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

// x = (q.x, q.y, qd.x, qd.y) of the sample, xm / xn of its neighbours t - 1 / t + 1 (read only where they exist)
// -> the sample's cost; g = d objective / d x.  At w_obj = 1, w = 0 the cost and g[0..1] are hinge_term's own bits.
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP>
__device__ __forceinline__ float traj_objective(const P2Hdr& S, const TrajPar& P, bool has_prev, bool has_next, const float4& x,
                                                const float4& xm, const float4& xn, float g[4]) {
    float hx, hy;
    const float h = hinge_term<GRID, ANALYTIC, WS, CLAMP>(S, make_float2(x.x, x.y), hx, hy);
    float acc = 0.0f, gpx, gvx, gpy, gvy;
    gp_coord(P, has_prev, has_next, x.x, x.z, xm.x, xm.z, xn.x, xn.z, acc, gpx, gvx);
    gp_coord(P, has_prev, has_next, x.y, x.w, xm.y, xm.w, xn.y, xn.w, acc, gpy, gvy);
    g[0] = fmaf(P.w_obj, hx, gpx); g[1] = fmaf(P.w_obj, hy, gpy); g[2] = gvx; g[3] = gvy;
    return fmaf(P.w_obj, h, P.w * acc);
}

// trk_scene2d_traj_cost_grad: any horizon; a lane takes its neighbours' rows with global loads of its own (the same cache lines
// its neighbour lanes load, so they cost issue slots and no traffic).
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP, bool GRAD>
__global__ void __launch_bounds__(256)
k_planar_traj_cost(P2Hdr S, TrajPar P, const float2* __restrict__ q, const float2* __restrict__ qd, int64_t n, int H,
                   float* __restrict__ cost, float2* __restrict__ gq, float2* __restrict__ gqd) {
    const int64_t base = (int64_t)blockIdx.x * 256;
    const int64_t s = base + threadIdx.x;
    if (s >= n) return;
    const unsigned t = ((unsigned)(base % H) + threadIdx.x) % (unsigned)H;         // the 64-bit remainder is uniform: scalar
    const bool has_prev = t > 0, has_next = t + 1 < (unsigned)H;
    const float2 p = q[s], v = qd[s];
    const float4 x = make_float4(p.x, p.y, v.x, v.y);
    float4 xm = x, xn = x;
    if (has_prev) { const float2 a = q[s - 1], b = qd[s - 1]; xm = make_float4(a.x, a.y, b.x, b.y); }
    if (has_next) { const float2 a = q[s + 1], b = qd[s + 1]; xn = make_float4(a.x, a.y, b.x, b.y); }
    float g[4];
    cost[s] = traj_objective<GRID, ANALYTIC, WS, CLAMP>(S, P, has_prev, has_next, x, xm, xn, g);
    if (GRAD) { gq[s] = make_float2(g[0], g[1]); gqd[s] = make_float2(g[2], g[3]); }
}

// trk_scene2d_traj_adam_steps: bias corrections of the iterations of one launch, by value like IkSchedule
constexpr int PLANAR_ADAM_MAX_STEPS = 32;
struct AdamPar {
    float lr; int32_t pin, n_steps, update;             // update == 0: evaluate only (cost), nothing else is written
    float bc1[PLANAR_ADAM_MAX_STEPS], rsqrt_bc2[PLANAR_ADAM_MAX_STEPS];
};

// trk_ik_step's Adam on one component
__device__ __forceinline__ void adam_component(float g, float step, float rsqrt_bc2, float& x, float& m, float& v) {
    const float m1 = fmaf(0.9f, m, 0.1f * g);
    const float v1 = fmaf(0.999f, v, 0.001f * g * g);
    m = m1; v = v1;
    const float denom = fmaf(sqrtf(v1), rsqrt_bc2, 1e-8f);
    x = x - step * (m1 / denom);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The via-point term (include/trk.h, trk_scene2d_traj_via_cost_grad): the hinge at the n interpolated points of the segment t -> t+1,
// attributed to sample t like the prior's factor.
// ---------------------------------------------------------------------------------------------------------------------------
struct ViaPar { float w_via; int32_t n; const float* alpha; const float* beta; };      // alpha, beta: device [n], the same for every lane

// The segment from x to xn: v[a] = x * alpha[a] + xn * beta[a], each product and the sum rounded once (k_planar_collision_via's
// arithmetic) -> c = sum_a h(v[a]), l = sum_a alpha[a] g(v[a]) (the segment's gradient on its own sample), u = sum_a beta[a] g(v[a])
// (on the next one); ascending a from 0.0f, c by plain adds, l and u by fmaf.  A run-time loop: the hinge's code is there once.
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP>
__device__ __forceinline__ void via_segment(const P2Hdr& S, const ViaPar& V, const float4& x, const float4& xn, float& c, float2& l,
                                            float2& u) {
    c = 0.0f; l = make_float2(0.0f, 0.0f); u = l;
    const TRK_CAS float* al = cptr(V.alpha);
    const TRK_CAS float* be = cptr(V.beta);
#pragma nounroll
    for (int a = 0; a < V.n; ++a) {
        const float wa = al[a], wb = be[a];
        const float px = __fadd_rn(__fmul_rn(x.x, wa), __fmul_rn(xn.x, wb));
        const float py = __fadd_rn(__fmul_rn(x.y, wa), __fmul_rn(xn.y, wb));
        float gx, gy;
        c = c + hinge_term<GRID, ANALYTIC, WS, CLAMP>(S, make_float2(px, py), gx, gy);
        l.x = fmaf(wa, gx, l.x); l.y = fmaf(wa, gy, l.y);
        u.x = fmaf(wb, gx, u.x); u.y = fmaf(wb, gy, u.y);
    }
}

// The persistent loop of the three entries (trk_scene2d_traj_adam_steps, trk_scene2d_traj_via_adam_steps and the one evaluation of
// trk_scene2d_traj_via_cost_grad: update == 0, which also stores the gradient), behind the two __global__ shells below.
// One lane per sample, a workgroup of 256 lanes owns floor(256 / H) whole trajectories (lanes beyond them idle); (q, qd, m, v) of a
// sample stay in its lane's registers for the n_steps iterations of the launch.  Each iteration a lane needs (q, qd) of t - 1 and t + 1:
//   WAVE (H == 64, a wavefront is a trajectory): two DPP wavefront shifts per value, no LDS and no barrier;
//   otherwise: through LDS, two buffers used in turn and ONE barrier per iteration -- a lane that writes buffer k & 1 for iteration
//   k + 2 has passed the barrier of iteration k + 1, which every lane reaches only after its reads of iteration k.
// VIA: the via term in the objective.  After the first exchange a lane with a segment (t < H - 1) walks the segment's n via points with
// (c, l, u) in registers, and u goes to lane t + 1:
//   WAVE: two more DPP shifts;
//   otherwise: one float2 per lane through LDS, ONE buffer and a second barrier per iteration.  A lane that writes uch for iteration
//   k + 1 has passed the first barrier of iteration k + 1, which every lane reaches only after its read of uch in iteration k; a
//   lane that reads uch in iteration k has passed the second barrier of iteration k, which every lane reaches only after its write.
//   With two barriers per iteration xch's two buffers are more than the first exchange needs; they stay as without the via term.
// Idle lanes (beyond the workgroup's whole trajectories, or beyond the batch) reach every barrier.  The lane without a segment and
// the lane without a predecessor have their shares removed by a select: what lane tid - 1 of another trajectory wrote never enters.
// The structs come by value, as the kernels take them: nothing is copied at run time, the fields stay scalar loads from the kernarg
// segment.  (By const& the compiler moved the grid cell's first use ahead of the workspace term in the grid + workspace + clamp
// variants, which exposes the gather's latency to a lone wavefront: 0.92 -> 1.02 us per iteration at 512 x 64 on EnvDense2D.)
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP, bool WAVE, bool VIA>
__device__ __forceinline__ void traj_loop(const P2Hdr S, const TrajPar P, const ViaPar V, const AdamPar A, float2* __restrict__ q,
                                          float2* __restrict__ qd, float4* __restrict__ mom, float4* __restrict__ vel, int64_t B, int H,
                                          float* __restrict__ cost, float2* __restrict__ gq, float2* __restrict__ gqd) {
    __shared__ float4 xch[WAVE ? 1 : 2][WAVE ? 1 : 256];
    __shared__ float2 uch[WAVE || !VIA ? 1 : 256];
    const int tid = threadIdx.x;
    const int per_wg = WAVE ? 4 : 256 / H;
    const int tl = WAVE ? tid >> 6 : tid / H;                      // the lane's trajectory within the workgroup
    const int t = WAVE ? tid & 63 : tid - tl * H;
    const int64_t traj = (int64_t)blockIdx.x * per_wg + tl;
    const bool active = tl < per_wg && traj < B;
    if (WAVE && !active) return;                                   // a whole wavefront: the DPP shifts below see all 64 lanes
    const int64_t s = traj * H + t;
    const bool has_prev = t > 0, has_next = t + 1 < H;
    const bool update = A.update != 0;
    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m = x, v = x;
    if (active) {
        const float2 a = q[s], b = qd[s];
        x = make_float4(a.x, a.y, b.x, b.y);
        if (update) { m = mom[s]; v = vel[s]; }
    }
    // a pinned component's gradient is taken as zero
    const bool pin_q = ((A.pin & 1) && t == 0) || ((A.pin & 2) && t == H - 1);
    const bool pin_qd = ((A.pin & 4) && t == 0) || ((A.pin & 8) && t == H - 1);
    for (int it = 0; it < A.n_steps; ++it) {
        float4 xm = x, xn = x;
        if (WAVE) {
            xm.x = trk_dpp_from_prev(x.x, x.x); xm.y = trk_dpp_from_prev(x.y, x.y);
            xm.z = trk_dpp_from_prev(x.z, x.z); xm.w = trk_dpp_from_prev(x.w, x.w);
            xn.x = trk_dpp_from_next(x.x, x.x); xn.y = trk_dpp_from_next(x.y, x.y);
            xn.z = trk_dpp_from_next(x.z, x.z); xn.w = trk_dpp_from_next(x.w, x.w);
        } else {
            xch[it & 1][tid] = x;
            __syncthreads();
            if (active && has_prev) xm = xch[it & 1][tid - 1];
            if (active && has_next) xn = xch[it & 1][tid + 1];
        }
        float vc = 0.0f;
        float2 vl = make_float2(0.0f, 0.0f), vu = vl, up = vl;
        if (VIA) {
            if (active && has_next) via_segment<GRID, ANALYTIC, WS, CLAMP>(S, V, x, xn, vc, vl, vu);
            if (WAVE) {
                up.x = trk_dpp_from_prev(0.0f, vu.x); up.y = trk_dpp_from_prev(0.0f, vu.y);
            } else {
                uch[tid] = vu;
                __syncthreads();
                if (active && has_prev) up = uch[tid - 1];
            }
            if (!has_prev) up = make_float2(0.0f, 0.0f);
        }
        if (active) {
            float g[4];
            float c = traj_objective<GRID, ANALYTIC, WS, CLAMP>(S, P, has_prev, has_next, x, xm, xn, g);
            if (VIA) {
                c = fmaf(V.w_via, vc, c);
                g[0] = fmaf(V.w_via, vl.x + up.x, g[0]); g[1] = fmaf(V.w_via, vl.y + up.y, g[1]);
            }
            if (it == 0 && cost) cost[s] = c;
            if (VIA && it == 0 && gq) { gq[s] = make_float2(g[0], g[1]); gqd[s] = make_float2(g[2], g[3]); }
            if (update) {
                const float step = A.lr / A.bc1[it], rs = A.rsqrt_bc2[it];
                adam_component(pin_q ? 0.0f : g[0], step, rs, x.x, m.x, v.x);
                adam_component(pin_q ? 0.0f : g[1], step, rs, x.y, m.y, v.y);
                adam_component(pin_qd ? 0.0f : g[2], step, rs, x.z, m.z, v.z);
                adam_component(pin_qd ? 0.0f : g[3], step, rs, x.w, m.w, v.w);
            }
        }
    }
    if (active && update) {
        q[s] = make_float2(x.x, x.y); qd[s] = make_float2(x.z, x.w);
        mom[s] = m; vel[s] = v;
    }
}

// the two shells keep their names and their kernel-argument segments: tools, tests and profiles find the kernels by them
template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP, bool WAVE>
__global__ void __launch_bounds__(256)
k_planar_traj_adam(P2Hdr S, TrajPar P, AdamPar A, float2* __restrict__ q, float2* __restrict__ qd, float4* __restrict__ mom,
                   float4* __restrict__ vel, int64_t B, int H, float* __restrict__ cost) {
    traj_loop<GRID, ANALYTIC, WS, CLAMP, WAVE, false>(S, P, ViaPar{}, A, q, qd, mom, vel, B, H, cost, nullptr, nullptr);
}

template <bool GRID, bool ANALYTIC, bool WS, bool CLAMP, bool WAVE>
__global__ void __launch_bounds__(256)
k_planar_traj_via(P2Hdr S, TrajPar P, ViaPar V, AdamPar A, float2* __restrict__ q, float2* __restrict__ qd, float4* __restrict__ mom,
                  float4* __restrict__ vel, int64_t B, int H, float* __restrict__ cost, float2* __restrict__ gq,
                  float2* __restrict__ gqd) {
    traj_loop<GRID, ANALYTIC, WS, CLAMP, WAVE, true>(S, P, V, A, q, qd, mom, vel, B, H, cost, gq, gqd);
}

template <bool GRID, bool ANALYTIC, bool WS>
__global__ void __launch_bounds__(256)
k_planar_collision(P2Hdr S, const float2* __restrict__ q, int64_t n, float m, uint8_t* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float2 p = q[s];
    out[s] = collides<GRID, ANALYTIC, WS>(S, m, p.x, p.y) ? 1 : 0;
}

// Via points: sample (t, i, a) = x[t, i] * alpha[a] + x[t, i + 1] * beta[a], each product and the sum rounded once, exactly as
// k_interpolate_via_points; the point is tested where it is formed and never stored.
template <bool GRID, bool ANALYTIC, bool WS>
__global__ void __launch_bounds__(256)
k_planar_collision_via(P2Hdr S, const float* __restrict__ x, int64_t total, int H, int SD, int n_interp,
                       const float* __restrict__ alpha, const float* __restrict__ beta, float m, uint8_t* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= total) return;
    const int per = (H - 1) * n_interp;
    const int64_t t = s / per;
    const int r = (int)(s - t * per);
    const int i = r / n_interp, a = r - i * n_interp;
    const float* w0 = x + (t * H + i) * (int64_t)SD;
    const float* w1 = w0 + SD;
    const float al = alpha[a], be = beta[a];
    const float px = __fadd_rn(__fmul_rn(w0[0], al), __fmul_rn(w1[0], be));
    const float py = __fadd_rn(__fmul_rn(w0[1], al), __fmul_rn(w1[1], be));
    out[s] = collides<GRID, ANALYTIC, WS>(S, m, px, py) ? 1 : 0;
}

// GridMapSDF.precompute_sdf in 2-D: min over the analytic objects with torch.minimum's gradient (ties share it evenly, folded in
// object order like the reference's running minimum).  One float4 store per cell.
__global__ void __launch_bounds__(256)
k_grid2d_precompute(P2Hdr S, int nx, int ny, float lo0, float lo1, float hi0, float hi1, float4* __restrict__ cells) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nx * ny) return;
    const int i = (int)(idx / ny), j = (int)(idx - (int64_t)i * ny);
    const float x = linspace_at(lo0, hi0, nx, i), y = linspace_at(lo1, hi1, ny, j);
    float best = __builtin_inff(), bx = 0.0f, by = 0.0f;
    for (int o = 0; o < S.n_objects; ++o) {
        float gx, gy;
        const float v = object2d_sdf(S, o, x, y, gx, gy);
        if (o == 0 || v < best) { best = v; bx = gx; by = gy; }
        else if (v == best) { bx = 0.5f * bx + 0.5f * gx; by = 0.5f * by + 0.5f * gy; }
    }
    cells[idx] = make_float4(best, bx, by, 0.0f);
}

__global__ void __launch_bounds__(256)
k_planar_sdf_points(P2Hdr S, const float2* __restrict__ pts, int64_t n, int n_df, float* __restrict__ sdf, float2* __restrict__ grad) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float2 p = pts[s];
    int k = 0;
    if (S.has_grid) {
        const float4 c = grid2d_cell(S, p.x, p.y);
        sdf[s * n_df] = c.x;
        if (grad) grad[s * n_df] = make_float2(c.y, c.z);
        k = 1;
    }
    for (int o = 0; o < S.n_objects; ++o, ++k) {
        float gx, gy;
        sdf[s * n_df + k] = object2d_sdf(S, o, p.x, p.y, gx, gy);
        if (grad) grad[s * n_df + k] = make_float2(gx, gy);
    }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// (grid, analytic, workspace) -> the compiled variant: f.go<G, A, W>()
template <class F>
void dispatch3(bool g, bool a, bool w, F&& f) {
    if (g) {
        if (a) { if (w) f.template go<true, true, true>(); else f.template go<true, true, false>(); }
        else   { if (w) f.template go<true, false, true>(); else f.template go<true, false, false>(); }
    } else {
        if (a) { if (w) f.template go<false, true, true>(); else f.template go<false, true, false>(); }
        else   { if (w) f.template go<false, false, true>(); else f.template go<false, false, false>(); }
    }
}

// two more run-time switches under a variant: f.launch<G, A, W, X, Y>()
template <bool G, bool A, bool W, class F>
void dispatch2(bool x, bool y, F& f) {
    if (x) { if (y) f.template launch<G, A, W, true, true>(); else f.template launch<G, A, W, true, false>(); }
    else { if (y) f.template launch<G, A, W, false, true>(); else f.template launch<G, A, W, false, false>(); }
}

// the launchers behind dispatch3: go<G, A, W>() starts that variant
struct CostGo {
    const P2Hdr& S; const float2* q; int64_t n; bool clamp; float* cost; float2* grad; hipStream_t st;
    template <bool G, bool A, bool W, bool C, bool GR> void launch() {
        hipLaunchKernelGGL((k_planar_cost<G, A, W, C, GR>), dim3(blocks_for(n)), dim3(256), 0, st, S, q, n, cost, grad);
    }
    template <bool G, bool A, bool W> void go() { dispatch2<G, A, W>(clamp, grad != nullptr, *this); }
};
struct CollGo {
    const P2Hdr& S; const float2* q; int64_t n; float m; uint8_t* out; hipStream_t st;
    template <bool G, bool A, bool W> void go() {
        hipLaunchKernelGGL((k_planar_collision<G, A, W>), dim3(blocks_for(n)), dim3(256), 0, st, S, q, n, m, out);
    }
};
struct ViaGo {
    const P2Hdr& S; const float* x; int64_t total; int H, SD, ni; const float* al; const float* be; float m; uint8_t* out; hipStream_t st;
    template <bool G, bool A, bool W> void go() {
        hipLaunchKernelGGL((k_planar_collision_via<G, A, W>), dim3(blocks_for(total)), dim3(256), 0, st, S, x, total, H, SD, ni, al, be, m, out);
    }
};
struct TrajCostGo {
    const P2Hdr& S; const TrajPar& P; const float2* q; const float2* qd; int64_t n; int H; bool clamp; float* cost; float2* gq; float2* gqd;
    hipStream_t st;
    template <bool G, bool A, bool W, bool C, bool GR> void launch() {
        hipLaunchKernelGGL((k_planar_traj_cost<G, A, W, C, GR>), dim3(blocks_for(n)), dim3(256), 0, st, S, P, q, qd, n, H, cost, gq, gqd);
    }
    template <bool G, bool A, bool W> void go() { dispatch2<G, A, W>(clamp, gq != nullptr, *this); }
};
// the two loop kernels: k_planar_traj_via where there is a via term (V), k_planar_traj_adam otherwise; a workgroup owns per_wg trajectories
struct TrajLoopGo {
    const P2Hdr& S; const TrajPar& P; const ViaPar* V; const AdamPar& Ad; float2* q; float2* qd; float4* m; float4* v; int64_t B; int H;
    bool clamp, wave; float* cost; float2* gq; float2* gqd; hipStream_t st;
    template <bool G, bool A, bool W, bool C, bool WV> void launch() {
        const int per_wg = WV ? 4 : 256 / H;
        const dim3 g((unsigned)((B + per_wg - 1) / per_wg)), b(256);
        if (V) hipLaunchKernelGGL((k_planar_traj_via<G, A, W, C, WV>), g, b, 0, st, S, P, *V, Ad, q, qd, m, v, B, H, cost, gq, gqd);
        else hipLaunchKernelGGL((k_planar_traj_adam<G, A, W, C, WV>), g, b, 0, st, S, P, Ad, q, qd, m, v, B, H, cost);
    }
    template <bool G, bool A, bool W> void go() { dispatch2<G, A, W>(clamp, wave, *this); }
};

}  // namespace

struct TrkScene2D {
    P2Hdr hdr{};
    P2Obj* d_objs = nullptr;
    P2Prim* d_prims = nullptr;
    float4* d_cells = nullptr;
    int n_df = 0;
    int has_ws = 0;
};

extern "C" {

int trk_scene2d_create(const TrkScene2DDesc* d, TrkScene2D** out) {
    if (!d || !out) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: null argument");
    if (d->abi_version != TRK_ABI_VERSION) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: abi_version mismatch");
    if (d->n_objects < 0 || d->n_objects > TRK_PLANAR_MAX_OBJECTS)
        return trk_fail(TRK_ERR_UNSUPPORTED, "trk_scene2d_create: n_objects out of range (0 .. TRK_PLANAR_MAX_OBJECTS)");
    if (d->n_prims < 0 || d->n_prims > TRK_PLANAR_MAX_PRIMS)
        return trk_fail(TRK_ERR_UNSUPPORTED, "trk_scene2d_create: n_prims out of range (0 .. TRK_PLANAR_MAX_PRIMS)");
    if ((d->n_objects > 0 && !d->objects) || (d->n_prims > 0 && !d->prims))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: null object / primitive table");
    for (int o = 0; o < d->n_objects; ++o) {
        const TrkObject2D& O = d->objects[o];
        if (O.prim_begin < 0 || O.prim_begin > O.prim_end || O.prim_end > d->n_prims)
            return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: object primitive range out of bounds");
    }
    for (int i = 0; i < d->n_prims; ++i) {
        const TrkPrim2D& P = d->prims[i];
        if (P.type != TRK_PRIM_SPHERE && P.type != TRK_PRIM_ROUNDED_BOX && P.type != TRK_PRIM_SHARP_BOX)
            return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: unknown primitive type");
    }
    if (d->has_grid) {
        if (!d->grid_cells || d->grid_dims[0] < 1 || d->grid_dims[1] < 1 || (int64_t)d->grid_dims[0] * d->grid_dims[1] > (1ll << 28) ||
            !(d->grid_map_dim[0] > 0.0f) || !(d->grid_map_dim[1] > 0.0f))
            return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: bad grid (cells, dims or map_dim)");
        if (reinterpret_cast<uintptr_t>(d->grid_cells) % 16)
            return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: grid_cells must be 16-byte aligned");
    }
    if (!std::isfinite(d->margin)) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_create: margin must be finite");
    int rc = trk_ensure_init();
    if (rc) return rc;

    TrkScene2D* s = new (std::nothrow) TrkScene2D();
    if (!s) return trk_fail(TRK_ERR_HIP, "trk_scene2d_create: out of host memory");
    std::vector<P2Obj> objs(d->n_objects > 0 ? d->n_objects : 1);
    std::vector<P2Prim> prims(d->n_prims > 0 ? d->n_prims : 1);
    for (int o = 0; o < d->n_objects; ++o) {
        const TrkObject2D& O = d->objects[o];
        P2Obj& D = objs[o];
        std::memset(&D, 0, sizeof(D));
        std::memcpy(D.pos, O.pos, sizeof(D.pos));
        std::memcpy(D.R, O.R, sizeof(D.R));
        D.begin = O.prim_begin; D.end = O.prim_end;
        const bool ident = O.R[0] == 1.0f && O.R[1] == 0.0f && O.R[2] == 0.0f && O.R[3] == 0.0f && O.R[4] == 1.0f &&
                           O.R[5] == 0.0f && O.R[6] == 0.0f && O.R[7] == 0.0f && O.R[8] == 1.0f;
        D.kind = !ident ? 2 : (O.pos[0] == 0.0f && O.pos[1] == 0.0f ? 0 : 1);
    }
    for (int i = 0; i < d->n_prims; ++i) {
        const TrkPrim2D& P = d->prims[i];
        P2Prim& D = prims[i];
        std::memset(&D, 0, sizeof(D));
        D.type = P.type; D.cx = P.center[0]; D.cy = P.center[1]; D.hx = P.half[0]; D.hy = P.half[1];
        D.r = P.type == TRK_PRIM_SHARP_BOX ? 0.0f : P.radius;
    }
    auto cleanup = [&](hipError_t e, const char* what) {
        if (s->d_objs) (void)hipFree(s->d_objs);
        if (s->d_prims) (void)hipFree(s->d_prims);
        if (s->d_cells) (void)hipFree(s->d_cells);
        delete s;
        return trk_hip_fail((int)e, what);
    };
    hipError_t e;
    if ((e = hipMalloc(&s->d_objs, sizeof(P2Obj) * objs.size())) != hipSuccess) return cleanup(e, "hipMalloc(objects)");
    if ((e = hipMalloc(&s->d_prims, sizeof(P2Prim) * prims.size())) != hipSuccess) return cleanup(e, "hipMalloc(prims)");
    if ((e = hipMemcpy(s->d_objs, objs.data(), sizeof(P2Obj) * objs.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return cleanup(e, "hipMemcpy(objects)");
    if ((e = hipMemcpy(s->d_prims, prims.data(), sizeof(P2Prim) * prims.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return cleanup(e, "hipMemcpy(prims)");
    P2Hdr& H = s->hdr;
    H.objs = s->d_objs; H.prims = s->d_prims; H.n_objects = d->n_objects;
    if (d->has_grid) {                                      // a snapshot, like trk_cost_model_create's grid
        const size_t bytes = sizeof(float4) * (size_t)d->grid_dims[0] * d->grid_dims[1];
        if ((e = hipMalloc(&s->d_cells, bytes)) != hipSuccess) return cleanup(e, "hipMalloc(grid)");
        if ((e = hipMemcpy(s->d_cells, d->grid_cells, bytes, hipMemcpyDeviceToDevice)) != hipSuccess) return cleanup(e, "hipMemcpy(grid)");
        H.cells = s->d_cells; H.has_grid = 1;
        H.nx = d->grid_dims[0]; H.ny = d->grid_dims[1];
        H.lim0 = d->grid_lim_min[0]; H.lim1 = d->grid_lim_min[1];
        H.md0 = d->grid_map_dim[0]; H.md1 = d->grid_map_dim[1];
        H.fd0 = (float)H.nx; H.fd1 = (float)H.ny;
    }
    s->has_ws = d->has_ws ? 1 : 0;
    H.ws_min0 = d->ws_min[0]; H.ws_min1 = d->ws_min[1]; H.ws_max0 = d->ws_max[0]; H.ws_max1 = d->ws_max[1];
    H.margin = d->margin;
    s->n_df = d->n_objects + (d->has_grid ? 1 : 0);
    *out = s;
    return TRK_OK;
}

void trk_scene2d_destroy(TrkScene2D* s) {
    if (!s) return;
    if (s->d_objs) (void)hipFree(s->d_objs);
    if (s->d_prims) (void)hipFree(s->d_prims);
    if (s->d_cells) (void)hipFree(s->d_cells);
    delete s;
}

static bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
// the tail of every entry: what the launch of `kernel` left behind
static int launched(const char* kernel) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRK_OK : trk_hip_fail((int)e, kernel);
}
// "<entry>: <what>" as the error text
static int fail_for(int code, const char* who, const char* what) {
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return trk_fail(code, msg);
}

int trk_scene2d_cost_grad(const TrkScene2D* s, const float* q, int64_t n, int32_t clamp, float* cost, float* grad, trk_stream_t stream) {
    if (!s || n < 0 || (n > 0 && (!q || !cost))) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_cost_grad: bad argument");
    if (!aligned_to(q, 8) || (grad && !aligned_to(grad, 8)))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_cost_grad: q and grad must be 8-byte aligned (one float2 per sample)");
    if (n == 0) return TRK_OK;
    CostGo f{s->hdr, (const float2*)q, n, clamp != 0, cost, (float2*)grad, (hipStream_t)stream};
    dispatch3(s->hdr.has_grid != 0, s->hdr.n_objects > 0, s->has_ws != 0, f);
    return launched("k_planar_cost");
}

int trk_scene2d_collision(const TrkScene2D* s, const float* q, int64_t n, float margin_override, uint8_t* out, trk_stream_t stream) {
    if (!s || n < 0 || (n > 0 && (!q || !out))) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_collision: bad argument");
    if (!aligned_to(q, 8)) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_collision: q must be 8-byte aligned");
    if (n == 0) return TRK_OK;
    const float m = std::isnan(margin_override) ? s->hdr.margin : margin_override;
    CollGo f{s->hdr, (const float2*)q, n, m, out, (hipStream_t)stream};
    dispatch3(s->hdr.has_grid != 0, s->hdr.n_objects > 0, s->has_ws != 0, f);
    return launched("k_planar_collision");
}

int trk_scene2d_collision_via(const TrkScene2D* s, const float* x, int64_t n_traj, int32_t horizon, int32_t state_dim, int32_t n_interp,
                              const float* alpha, const float* beta, float margin_override, uint8_t* out, trk_stream_t stream) {
    if (!s || n_traj < 0 || horizon < 2 || state_dim < 2 || n_interp < 1 || !alpha || !beta || (n_traj > 0 && (!x || !out)))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_collision_via: bad argument");
    if ((int64_t)(horizon - 1) * n_interp > (1ll << 30) || (int64_t)horizon * state_dim > (1ll << 30))
        return trk_fail(TRK_ERR_UNSUPPORTED, "trk_scene2d_collision_via: trajectory too long");
    if (n_traj == 0) return TRK_OK;
    const float m = std::isnan(margin_override) ? s->hdr.margin : margin_override;
    const int64_t total = n_traj * (int64_t)(horizon - 1) * n_interp;
    ViaGo f{s->hdr, x, total, horizon, state_dim, n_interp, alpha, beta, m, out, (hipStream_t)stream};
    dispatch3(s->hdr.has_grid != 0, s->hdr.n_objects > 0, s->has_ws != 0, f);
    return launched("k_planar_collision_via");
}

int trk_grid2d_precompute(const TrkScene2D* s, const int32_t dims[2], const float lim_min[2], const float lim_max[2], float* cells,
                          trk_stream_t stream) {
    if (!s || !dims || !lim_min || !lim_max || !cells) return trk_fail(TRK_ERR_INVALID_ARG, "trk_grid2d_precompute: null argument");
    if (dims[0] < 1 || dims[1] < 1 || (int64_t)dims[0] * dims[1] > (1ll << 28))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_grid2d_precompute: bad dims");
    if (!aligned_to(cells, 16)) return trk_fail(TRK_ERR_INVALID_ARG, "trk_grid2d_precompute: cells must be 16-byte aligned");
    if (s->hdr.n_objects < 1) return trk_fail(TRK_ERR_INVALID_ARG, "trk_grid2d_precompute: the scene has no analytic objects");
    const int64_t total = (int64_t)dims[0] * dims[1];
    hipLaunchKernelGGL(k_grid2d_precompute, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, s->hdr, dims[0], dims[1],
                       lim_min[0], lim_min[1], lim_max[0], lim_max[1], (float4*)cells);
    return launched("k_grid2d_precompute");
}

int trk_scene2d_sdf_points(const TrkScene2D* s, const float* points, int64_t n, float* sdf, float* grad, trk_stream_t stream) {
    if (!s || n < 0 || (n > 0 && (!points || !sdf))) return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_sdf_points: bad argument");
    if (!aligned_to(points, 8) || (grad && !aligned_to(grad, 8)))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_sdf_points: points and grad must be 8-byte aligned");
    if (n == 0 || s->n_df == 0) return TRK_OK;
    hipLaunchKernelGGL(k_planar_sdf_points, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, s->hdr, (const float2*)points, n,
                       s->n_df, sdf, (float2*)grad);
    return launched("k_planar_sdf_points");
}

// What the trajectory entry points ask of their common arguments, before anything is dereferenced or launched; fills P.
static int check_traj_call(const char* who, const TrkScene2D* s, const TrkPlanarObjective* o, int64_t batch, int32_t horizon, TrajPar& P) {
    const char* bad = nullptr;
    if (!s || !o) bad = "null scene / objective";
    else if (batch < 0 || horizon < 1) bad = "batch must be >= 0 and horizon >= 1";
    else if (!(o->gp.dt > 0.0f) || !std::isfinite(o->gp.dt) || !(o->gp.sigma > 0.0f) || !std::isfinite(o->gp.sigma))
        bad = "the prior needs finite dt > 0 and sigma > 0";
    else if (!std::isfinite(o->w_obj) || !std::isfinite(o->gp.weight)) bad = "w_obj and gp.weight must be finite";
    if (bad) return fail_for(TRK_ERR_INVALID_ARG, who, bad);
    if (batch > 0x7fffffff || (batch * (int64_t)horizon + 255) / 256 > 0x7fffffff)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "batch x horizon too large");
    const float dt = o->gp.dt, s2 = 1.0f / (o->gp.sigma * o->gp.sigma);               // as trk_launch_gp_prior forms them
    P = TrajPar{o->w_obj, dt, 12.0f * s2 / (dt * dt * dt), -6.0f * s2 / (dt * dt), 4.0f * s2 / dt, o->gp.weight};
    return TRK_OK;
}

// What both via entry points ask on top of check_traj_call, before anything is dereferenced or launched; fills P and V.
static int check_via_call(const char* who, const TrkScene2D* s, const TrkPlanarViaObjective* o, int64_t batch, int32_t horizon, TrajPar& P,
                          ViaPar& V) {
    if (!o) return fail_for(TRK_ERR_INVALID_ARG, who, "null TrkPlanarViaObjective");
    int rc = check_traj_call(who, s, &o->base, batch, horizon, P);
    if (rc) return rc;
    if (!std::isfinite(o->w_via) || o->n_interp < 1 || !o->alpha || !o->beta)
        return fail_for(TRK_ERR_INVALID_ARG, who, "w_via must be finite, n_interp >= 1 and alpha, beta device arrays of n_interp weights");
    if (horizon > TRK_PLANAR_MAX_HORIZON)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "horizon above TRK_PLANAR_MAX_HORIZON (256): a workgroup owns whole trajectories");
    V = ViaPar{o->w_via, o->n_interp, o->alpha, o->beta};
    return TRK_OK;
}

// The two checks of the loop entries.  Each entry places them among its other checks itself: the via entry looks at the TrkPlanarAdam
// before check_via_call, the plain one after check_traj_call (and at its horizon limit last) -- the order a caller sees.
static int check_planar_adam(const char* who, const TrkPlanarAdam* ad) {
    if (!ad) return fail_for(TRK_ERR_INVALID_ARG, who, "null TrkPlanarAdam");
    if (ad->n_steps < 0 || ad->first_step < 1 || !std::isfinite(ad->lr) || ad->pin < 0 || ad->pin > 15)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_steps >= 0, first_step >= 1, lr finite and pin in 0 .. 15");
    return TRK_OK;
}
static bool planar_adam_updates(const TrkPlanarAdam* ad) { return ad->lr != 0.0f && ad->n_steps > 0; }
// the state buffers: adam_m, adam_v may be null where nothing is updated
static int check_state_buffers(const char* who, const TrkPlanarAdam* ad, const float* q, const float* qd, const float* adam_m,
                               const float* adam_v, int64_t batch) {
    if (batch > 0 && (!q || !qd || (planar_adam_updates(ad) && (!adam_m || !adam_v))))
        return fail_for(TRK_ERR_INVALID_ARG, who, "null q / qd / adam_m / adam_v");
    if (!aligned_to(q, 8) || !aligned_to(qd, 8) || !aligned_to(adam_m, 16) || !aligned_to(adam_v, 16))
        return fail_for(TRK_ERR_INVALID_ARG, who, "q, qd must be 8-byte and adam_m, adam_v 16-byte aligned");
    return TRK_OK;
}

// H == 64: a wavefront is a trajectory and the neighbours come by DPP; TRK_PLANAR_ADAM_LDS64=1 runs the LDS form there too
// (the same arithmetic, for measuring one exchange against the other)
static bool wave_form(int32_t horizon) {
    static const bool lds64 = [] { const char* v = getenv("TRK_PLANAR_ADAM_LDS64"); return v && v[0] == '1'; }();
    return horizon == 64 && !lds64;
}

// The launches of a call to one of the three loop entries (V: the via term, or null for the plain loop): at most PLANAR_ADAM_MAX_STEPS
// iterations each, with their slice of the bias-correction schedule; cost (and gq, gqd) come from the first launch, the state as the
// caller passed it.  Without an update it is one evaluation.
static int run_traj_loop(const TrkScene2D* s, const TrajPar& P, const ViaPar* V, bool clamp, const TrkPlanarAdam& ad, float* q, float* qd,
                         float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost, float* gq, float* gqd,
                         trk_stream_t stream) {
    const bool update = planar_adam_updates(&ad);
    const int32_t total = update ? ad.n_steps : 1;
    for (int32_t done = 0; done < total; done += PLANAR_ADAM_MAX_STEPS) {
        AdamPar A{};
        A.lr = ad.lr; A.pin = ad.pin; A.update = update ? 1 : 0;
        A.n_steps = std::min<int32_t>(PLANAR_ADAM_MAX_STEPS, total - done);
        trk_adam_bias_schedule(A.bc1, A.rsqrt_bc2, (int64_t)ad.first_step + done, A.n_steps);
        const bool first = done == 0;
        TrajLoopGo f{s->hdr, P, V, A, (float2*)q, (float2*)qd, (float4*)adam_m, (float4*)adam_v, batch, horizon, clamp, wave_form(horizon),
                     first ? cost : nullptr, (float2*)(first ? gq : nullptr), (float2*)(first ? gqd : nullptr), (hipStream_t)stream};
        dispatch3(s->hdr.has_grid != 0, s->hdr.n_objects > 0, s->has_ws != 0, f);
        if (int rc = launched(V ? "k_planar_traj_via" : "k_planar_traj_adam")) return rc;
    }
    return TRK_OK;
}

int trk_scene2d_traj_cost_grad(const TrkScene2D* s, const TrkPlanarObjective* o, const float* q, const float* qd, int64_t batch,
                               int32_t horizon, float* cost, float* gq, float* gqd, trk_stream_t stream) {
    const char* who = "trk_scene2d_traj_cost_grad";
    TrajPar P;
    int rc = check_traj_call(who, s, o, batch, horizon, P);
    if (rc) return rc;
    if ((batch > 0 && (!q || !qd || !cost)) || (gq == nullptr) != (gqd == nullptr))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_traj_cost_grad: null q / qd / cost, or only one of gq / gqd");
    if (!aligned_to(q, 8) || !aligned_to(qd, 8) || !aligned_to(gq, 8) || !aligned_to(gqd, 8))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_traj_cost_grad: q, qd, gq and gqd must be 8-byte aligned (one float2 per sample)");
    if (batch == 0) return TRK_OK;
    TrajCostGo f{s->hdr, P, (const float2*)q, (const float2*)qd, batch * horizon, horizon, o->clamp != 0, cost, (float2*)gq, (float2*)gqd,
                 (hipStream_t)stream};
    dispatch3(s->hdr.has_grid != 0, s->hdr.n_objects > 0, s->has_ws != 0, f);
    return launched("k_planar_traj_cost");
}

int trk_scene2d_traj_adam_steps(const TrkScene2D* s, const TrkPlanarObjective* o, const TrkPlanarAdam* ad, float* q, float* qd,
                                float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost, trk_stream_t stream) {
    const char* who = "trk_scene2d_traj_adam_steps";
    TrajPar P;
    int rc = check_traj_call(who, s, o, batch, horizon, P);
    if (!rc) rc = check_planar_adam(who, ad);
    if (!rc) rc = check_state_buffers(who, ad, q, qd, adam_m, adam_v, batch);
    if (rc) return rc;
    if (horizon > TRK_PLANAR_MAX_HORIZON)
        return trk_fail(TRK_ERR_UNSUPPORTED, "trk_scene2d_traj_adam_steps: horizon above TRK_PLANAR_MAX_HORIZON (256): a workgroup owns "
                                             "whole trajectories; trk_scene2d_traj_cost_grad serves any horizon");
    if (batch == 0 || (!planar_adam_updates(ad) && !cost)) return TRK_OK;
    return run_traj_loop(s, P, nullptr, o->clamp != 0, *ad, q, qd, adam_m, adam_v, batch, horizon, cost, nullptr, nullptr, stream);
}

int trk_scene2d_traj_via_cost_grad(const TrkScene2D* s, const TrkPlanarViaObjective* o, const float* q, const float* qd, int64_t batch,
                                   int32_t horizon, float* cost, float* gq, float* gqd, trk_stream_t stream) {
    const char* who = "trk_scene2d_traj_via_cost_grad";
    TrajPar P;
    ViaPar V;
    if ((batch > 0 && (!q || !qd || !cost)) || (gq == nullptr) != (gqd == nullptr))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_traj_via_cost_grad: null q / qd / cost, or only one of gq / gqd");
    int rc = check_via_call(who, s, o, batch, horizon, P, V);
    if (rc) return rc;
    if (!aligned_to(q, 8) || !aligned_to(qd, 8) || !aligned_to(gq, 8) || !aligned_to(gqd, 8))
        return trk_fail(TRK_ERR_INVALID_ARG, "trk_scene2d_traj_via_cost_grad: q, qd, gq and gqd must be 8-byte aligned (one float2 per sample)");
    if (batch == 0) return TRK_OK;
    // one evaluation: no update, nothing but cost, gq and gqd is written (q, qd are read only)
    const TrkPlanarAdam once{0.0f, 0, 1, 1};
    return run_traj_loop(s, P, &V, o->base.clamp != 0, once, const_cast<float*>(q), const_cast<float*>(qd), nullptr, nullptr, batch, horizon,
                         cost, gq, gqd, stream);
}

int trk_scene2d_traj_via_adam_steps(const TrkScene2D* s, const TrkPlanarViaObjective* o, const TrkPlanarAdam* ad, float* q, float* qd,
                                    float* adam_m, float* adam_v, int64_t batch, int32_t horizon, float* cost, trk_stream_t stream) {
    const char* who = "trk_scene2d_traj_via_adam_steps";
    TrajPar P;
    ViaPar V;
    int rc = check_planar_adam(who, ad);
    if (!rc) rc = check_via_call(who, s, o, batch, horizon, P, V);
    if (!rc) rc = check_state_buffers(who, ad, q, qd, adam_m, adam_v, batch);
    if (rc) return rc;
    if (batch == 0 || (!planar_adam_updates(ad) && !cost)) return TRK_OK;
    return run_traj_loop(s, P, &V, o->base.clamp != 0, *ad, q, qd, adam_m, adam_v, batch, horizon, cost, nullptr, nullptr, stream);
}

}  // extern "C"

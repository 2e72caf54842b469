// trk_gp_sample.hip -- multi-particle planning (include/trk.h, "GP-prior sampling and best-particle pick"): trajectories drawn from
// the start/goal-conditioned constant-velocity GP prior (trk_gp_prior_sample: the prior whose cost is trk_gp_prior_cost_grad) and the
// pick of one particle per problem (trk_traj_select_best).  Kernels and their C entries; the noise is an input, nothing here draws.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include "trk_launch.h"

namespace {

// One launch's constants, by value (scalar loads from the kernarg segment).  l00, l10, l11: the Cholesky factor of the prior's Q;
// theta = (H - 1) dt.  All formed in double on the host and rounded once.
struct GpSamplePar {
    float dt, l00, l10, l11, theta;
    int32_t pin_vel, has_lim;
};

// An element of the workgroup's tile is (trajectory tl of the workgroup, sample t, coordinate d), packed t | d << 8 | tl << 16; -1 for
// a lane's slot beyond the tile.
__device__ __forceinline__ int el_t(int pack) { return pack & 255; }
__device__ __forceinline__ int el_d(int pack) { return (pack >> 8) & 255; }
__device__ __forceinline__ int el_tl(int pack) { return pack >> 16; }
// the problem of trajectory j0 + tl (below 2^30: a 32-bit division)
__device__ __forceinline__ int64_t problem_of(int64_t j0, int tl, int K) { return (int64_t)((uint32_t)(j0 + tl) / (uint32_t)K); }

// Inclusive sum along t of every (trajectory, coordinate) of the tile, in place in the lanes' registers: Hillis-Steele through LDS,
// x[t] = x[t - off] + x[t] for off = 1, 2, 4, ... < H.  The partner is a select on t >= off, so nothing crosses from the trajectory
// before, and the association of a sum depends on t alone: not on the trajectory's place in the tile or in the batch.
// Leaves with the last read of xch behind a barrier.
template <int EMAX, int LANES>
__device__ __forceinline__ void scan_along_t(float* xch, const int (&pack)[EMAX], float (&x)[EMAX], int E, int H, int D, int tid) {
    for (int off = 1; off < H; off <<= 1) {
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E && pack[e] >= 0) xch[e * LANES + tid] = x[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EMAX; ++e)
            if (e < E && pack[e] >= 0 && el_t(pack[e]) >= off) x[e] = xch[e * LANES + tid - off * D] + x[e];
        __syncthreads();
    }
}

// A workgroup owns floor(256 / H) whole trajectories (k_point3d_traj's split), which are one contiguous run of q, qd and eps: a tile
// of at most 256 D elements.  The run is dealt to the lanes element by element -- element i = e * LANES + tid of the tile is (row
// i / D, coordinate i % D) -- so every global access of a wavefront covers 64 consecutive elements, and a lane keeps its <= EMAX
// elements in registers (the loops over e are unrolled; E, the number in use, is uniform).  LANES = 256 up to 8 coordinates; 512 and
// 1024 lanes keep EMAX at 8 up to 16 and 32 coordinates (32 elements a lane do not fit the register file without scratch).  The
// two sums along t run over the tile in LDS (scan_along_t).
//   a[t] = v_0 at t = 0, w^v_{t-1} after          -> v[t]  = a[0] + ... + a[t]
//   b[t] = start at t = 0, dt v[t-1] + w^p_{t-1}  -> p[t]  = b[0] + ... + b[t]
// then p[H-1] (and v[H-1]) of the trajectory condition every sample, the endpoints are selected and the interior is clamped.
template <int EMAX, int LANES>
__global__ void __launch_bounds__(LANES)
k_gp_sample(const GpSamplePar P, const float* __restrict__ start, const float* __restrict__ goal, const float* __restrict__ start_vel,
            const float* __restrict__ goal_vel, const float* __restrict__ eps, const float* __restrict__ q_min,
            const float* __restrict__ q_max, int K, int64_t n_traj, int H, int D, float* __restrict__ q, float* __restrict__ qd) {
    __shared__ float xch[LANES * EMAX];
    const int tid = threadIdx.x;
    const int per_wg = 256 / H;
    const int64_t j0 = (int64_t)blockIdx.x * per_wg;
    const int64_t left = n_traj - j0;
    const int n_here = left < per_wg ? (int)left : per_wg;
    const int M = n_here * H * D;                                  // <= 256 D elements
    const int E = (M + LANES - 1) / LANES;                         // <= EMAX: 256 D <= LANES * EMAX
    const int T = H - 1;
    const int64_t base = j0 * H * D;                               // of the tile in q, qd
    const int64_t ebase = j0 * T * D;                              // of the tile in eps, in (e0, e1) pairs
    const bool eps8 = (reinterpret_cast<uintptr_t>(eps) & 7) == 0;

    int pack[EMAX];
    float v[EMAX], x[EMAX];
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        pack[e] = -1; v[e] = 0.0f; x[e] = 0.0f;
        if (e < E) {
            const int i = e * LANES + tid;
            if (i < M) {
                const int r = i / D, d = i - r * D;
                const int tl = r / H, t = r - tl * H;
                pack[e] = t | (d << 8) | (tl << 16);
                if (t == 0) {
                    const int64_t pd = problem_of(j0, tl, K) * D + d;
                    v[e] = P.pin_vel ? start_vel[pd] : 0.0f;
                    x[e] = start[pd];
                } else {
                    const int64_t at = ebase + ((int64_t)tl * T + (t - 1)) * D + d;
                    float e0, e1;
                    if (eps8) { const float2 ee = reinterpret_cast<const float2*>(eps)[at]; e0 = ee.x; e1 = ee.y; }
                    else { e0 = eps[2 * at]; e1 = eps[2 * at + 1]; }
                    v[e] = P.l10 * e0 + P.l11 * e1;                // w^v of the step t-1 -> t
                    x[e] = P.l00 * e0;                             // w^p of the same step
                }
            }
        }
    }
    scan_along_t<EMAX, LANES>(xch, pack, v, E, H, D, tid);
    // b[t] = dt v[t-1] + w^p_{t-1}: v of the sample before, through LDS
#pragma unroll
    for (int e = 0; e < EMAX; ++e)
        if (e < E && pack[e] >= 0) xch[e * LANES + tid] = v[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EMAX; ++e)
        if (e < E && pack[e] >= 0 && el_t(pack[e]) > 0) x[e] = P.dt * xch[e * LANES + tid - D] + x[e];
    __syncthreads();
    scan_along_t<EMAX, LANES>(xch, pack, x, E, H, D, tid);
    // p[T] and v[T] of every (trajectory, coordinate), from the lane that holds them: the two halves of xch (a workgroup owns at most
    // 128 trajectories, 128 D <= LANES * EMAX / 2 floats each)
    float* const pTs = xch;
    float* const vTs = xch + LANES * EMAX / 2;
#pragma unroll
    for (int e = 0; e < EMAX; ++e)
        if (e < E && pack[e] >= 0 && el_t(pack[e]) == T) {
            pTs[el_tl(pack[e]) * D + el_d(pack[e])] = x[e];
            vTs[el_tl(pack[e]) * D + el_d(pack[e])] = v[e];
        }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        if (e < E && pack[e] >= 0) {
            const int t = el_t(pack[e]), d = el_d(pack[e]), tl = el_tl(pack[e]);
            const int64_t pd = problem_of(j0, tl, K) * D + d;
            const float g = goal[pd];
            const float rp = g - pTs[tl * D + d];
            float qo, qdo;
            if (P.pin_vel) {
                const float s = (float)t / (float)T;
                const float rv = goal_vel[pd] - vTs[tl * D + d];
                const float s2 = s * s;
                const float h_pp = s2 * (3.0f - 2.0f * s);         // 3 s^2 - 2 s^3
                const float h_pv = P.theta * (s2 * (s - 1.0f));    // theta (s^3 - s^2)
                const float h_vp = (6.0f * s) * (1.0f - s) / P.theta;
                const float h_vv = s * (3.0f * s - 2.0f);          // 3 s^2 - 2 s
                qo = x[e] + h_pp * rp + h_pv * rv;
                qdo = v[e] + h_vp * rp + h_vv * rv;
                if (t == 0) qdo = start_vel[pd];
                if (t == T) qdo = goal_vel[pd];
            } else {
                const float vs = rp / P.theta;
                qo = x[e] + ((float)t * P.dt) * vs;
                qdo = v[e] + vs;
            }
            if (P.has_lim) {                                       // comparisons, not fmin / fmax: a NaN stays a NaN
                const float lo = q_min[d], hi = q_max[d];
                qo = qo < lo ? lo : (qo > hi ? hi : qo);
            }
            if (t == 0) qo = start[pd];
            if (t == T) qo = g;
            q[base + e * LANES + tid] = qo;
            qd[base + e * LANES + tid] = qdo;
        }
    }
}

// One group of G lanes (a power of two <= 64, inside one wavefront) per problem, 256 / G problems per workgroup: a lane walks the
// particles k = l, l + G, ... in ascending order and keeps the first smallest score, then the group folds by xor shuffles; between
// equal scores the smaller k wins at every fold, so the result is the first smallest in k whatever G is.  NONE: no candidate yet.
constexpr int NONE = 0x7fffffff;
__global__ void __launch_bounds__(256)
k_select_best(const float* __restrict__ score, const uint8_t* __restrict__ is_free, int64_t n_problems, int K, int G,
              int64_t* __restrict__ best, float* __restrict__ best_score, int32_t* __restrict__ n_free) {
    const int tid = threadIdx.x;
    const int l = tid & (G - 1);
    const int64_t p = (int64_t)blockIdx.x * (256 / G) + tid / G;
    const bool active = p < n_problems;
    float bs = INFINITY;
    int bk = NONE, cnt = 0;
    if (active) {
        for (int k = l; k < K; k += G) {
            const bool fr = is_free ? is_free[p * K + k] != 0 : true;
            const float s = score[p * K + k];
            cnt += fr ? 1 : 0;
            if (fr && !(s != s) && (bk == NONE || s < bs)) { bs = s; bk = k; }
        }
    }
    for (int m = G >> 1; m >= 1; m >>= 1) {                        // every lane of the wavefront takes part
        const float os = __shfl_xor(bs, m);
        const int ok = __shfl_xor(bk, m);
        cnt += __shfl_xor(cnt, m);
        if (ok != NONE && (bk == NONE || os < bs || (os == bs && ok < bk))) { bs = os; bk = ok; }
    }
    if (active && l == 0) {
        best[p] = bk == NONE ? (int64_t)-1 : p * K + bk;
        if (best_score) best_score[p] = bk == NONE ? INFINITY : bs;
        if (n_free) n_free[p] = cnt;
    }
}

int launched(const char* kernel) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRK_OK : trk_hip_fail((int)e, kernel);
}
int fail_for(int code, const char* who, const char* what) {
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return trk_fail(code, msg);
}

}  // namespace

extern "C" {

int trk_gp_prior_sample(const TrkGpSample* s, const float* start, const float* goal, const float* start_vel, const float* goal_vel,
                        const float* eps, const float* q_min, const float* q_max, int64_t n_problems, int32_t horizon, int32_t dof,
                        float* q, float* qd, trk_stream_t stream) {
    const char* who = "trk_gp_prior_sample";
    if (!s) return fail_for(TRK_ERR_INVALID_ARG, who, "null TrkGpSample");
    if (!std::isfinite(s->dt) || !std::isfinite(s->sigma) || !(s->dt > 0.0f) || !(s->sigma > 0.0f))
        return fail_for(TRK_ERR_INVALID_ARG, who, "dt and sigma must be finite and > 0");
    if (s->n_particles < 1 || (s->pin_vel != 0 && s->pin_vel != 1))
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_particles must be >= 1 and pin_vel 0 or 1");
    if (n_problems < 0 || horizon < 2 || dof < 1) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems >= 0, horizon >= 2 and dof >= 1");
    if (n_problems > 0x3fffffff / s->n_particles)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * n_particles above 0x3fffffff");
    if (n_problems > 0 && (!start || !goal || !eps || !q || !qd)) return fail_for(TRK_ERR_INVALID_ARG, who, "null start / goal / eps / q / qd");
    if (s->pin_vel && (!start_vel || !goal_vel)) return fail_for(TRK_ERR_INVALID_ARG, who, "pin_vel needs start_vel and goal_vel");
    if ((q_min == nullptr) != (q_max == nullptr)) return fail_for(TRK_ERR_INVALID_ARG, who, "only one of q_min / q_max");
    if (horizon > TRK_GP_SAMPLE_MAX_HORIZON)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "horizon above TRK_GP_SAMPLE_MAX_HORIZON (256): a workgroup owns whole trajectories");
    if (dof > TRK_GP_SAMPLE_MAX_DOF)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "dof above TRK_GP_SAMPLE_MAX_DOF (32): the tile of a workgroup is at most 256 x 32 elements");
    if (n_problems == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    GpSamplePar P;
    const double dt = s->dt, sg = s->sigma;
    P.dt = s->dt;
    P.l00 = (float)(sg * dt * std::sqrt(dt) / std::sqrt(3.0));
    P.l10 = (float)(sg * (std::sqrt(3.0) / 2.0) * std::sqrt(dt));
    P.l11 = (float)(sg * std::sqrt(dt) / 2.0);
    P.theta = (float)((double)(horizon - 1) * dt);
    P.pin_vel = s->pin_vel; P.has_lim = q_min != nullptr;
    const int64_t n_traj = n_problems * s->n_particles;
    const int per_wg = 256 / horizon;
    const dim3 g((unsigned)((n_traj + per_wg - 1) / per_wg));
    hipStream_t st = (hipStream_t)stream;
#define TRK_GP_SAMPLE_GO(EMAX, LANES) hipLaunchKernelGGL((k_gp_sample<EMAX, LANES>), g, dim3(LANES), 0, st, P, start, goal, start_vel, \
                                                         goal_vel, eps, q_min, q_max, s->n_particles, n_traj, horizon, dof, q, qd)
    if (dof <= 4) TRK_GP_SAMPLE_GO(4, 256);
    else if (dof <= 8) TRK_GP_SAMPLE_GO(8, 256);
    else if (dof <= 16) TRK_GP_SAMPLE_GO(8, 512);
    else TRK_GP_SAMPLE_GO(8, 1024);
#undef TRK_GP_SAMPLE_GO
    return launched("k_gp_sample");
}

int trk_traj_select_best(const float* score, const uint8_t* is_free, int64_t n_problems, int32_t n_particles, int64_t* best,
                         float* best_score, int32_t* n_free, trk_stream_t stream) {
    const char* who = "trk_traj_select_best";
    if (n_problems < 0 || n_particles < 1) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems >= 0 and n_particles >= 1");
    if (n_problems > 0x3fffffff / n_particles) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * n_particles above 0x3fffffff");
    if (n_problems > 0 && (!score || !best)) return fail_for(TRK_ERR_INVALID_ARG, who, "null score / best");
    if (n_problems == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    int G = 1;
    while (G < n_particles && G < 64) G <<= 1;
    const int per_wg = 256 / G;
    const dim3 g((unsigned)((n_problems + per_wg - 1) / per_wg)), b(256);
    hipLaunchKernelGGL(k_select_best, g, b, 0, (hipStream_t)stream, score, is_free, n_problems, n_particles, G, best, best_score, n_free);
    return launched("k_select_best");
}

}  // extern "C"

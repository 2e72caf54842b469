// trk_traj_post.hip -- trajectory post-processing (include/trk.h, "Trajectory post-processing"): the clamped cubic spline through a
// path, resampled to positions and velocities (trk_traj_spline_resample: the reference's smoothen_trajectory), and the variance of
// the particles' pairwise distances per way point (trk_traj_waypoint_variance: compute_variance_waypoints).  Kernels and C entries.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include "trk_launch.h"

namespace {

constexpr int SPLINE_LANES = 256;
constexpr int SPLINE_PIVOTS = 32;                  // m_i has converged to 2 - sqrt(3) in double long before i = 32
constexpr int SPLINE_TILE_BYTES = 64 * 1024;       // y and the slopes of a workgroup's trajectories: two workgroups fit a CU's 160 KiB
constexpr int SPLINE_FILL_GRID = 512;              // below this many workgroups a smaller tile is better than an idle CU

// One launch's constants, by value.  h = 1 / (N - 1), sdt = S dt and the pivots m_1 = 1/4, m_i = 1 / (4 - m_{i-1}) are formed in double
// on the host and rounded once; c3 = 3 (N - 1) and c6 = 6 (N - 1) are exact.
struct SplinePar {
    float h, c3, c6, sdt;
    int32_t vel_mode;
    float piv[SPLINE_PIVOTS];
};

// A workgroup owns per_wg whole trajectories (k_gp_sample's split): one contiguous run of y, pos and vel, loaded and stored element by
// element, so every global access of a wavefront covers 64 consecutive floats for any D.  LDS: the tile ys[n N D], the slopes
// ss[n N D] at the same indices, and the samples' (segment, tau) table.  One lane per (trajectory, coordinate) column runs the two
// Thomas sweeps down its column -- consecutive coordinates are consecutive LDS words -- so a column's bits depend on its own inputs
// alone.  Then the n S D outputs are dealt to all lanes.
__global__ void __launch_bounds__(SPLINE_LANES)
k_spline_resample(const SplinePar P, const float* __restrict__ y, int64_t n_traj, int per_wg, int N, int D, int S,
                  float* __restrict__ pos, float* __restrict__ vel) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * per_wg;
    const int64_t left = n_traj - j0;
    const int n_here = left < per_wg ? (int)left : per_wg;
    const int ND = N * D;
    const int M = n_here * ND;
    float* const ys = lds;
    float* const ss = lds + per_wg * ND;
    int* const seg = reinterpret_cast<int*>(lds + 2 * per_wg * ND);
    float* const taus = lds + 2 * per_wg * ND + S;

    const float* const yin = y + j0 * ND;
    for (int e = tid; e < M; e += SPLINE_LANES) ys[e] = yin[e];
    // sample k: a = k (N - 1), segment a / (S - 1), tau = (a % (S - 1)) / (S - 1); the last one is the end of segment N - 2
    for (int k = tid; k < S; k += SPLINE_LANES) {
        const int a = k * (N - 1);
        const int i = a / (S - 1), r = a - i * (S - 1);
        const bool last = k == S - 1;
        seg[k] = last ? N - 2 : i;
        taus[k] = last ? 1.0f : (float)r / (float)(S - 1);
    }
    __syncthreads();

    // s_0 = s_{N-1} = 0;  s_{i-1} + 4 s_i + s_{i+1} = 3 (N - 1) (y_{i+1} - y_{i-1}):  g_i = (b_i - g_{i-1}) m_i down, s_i = g_i - m_i s_{i+1} up
    for (int col = tid; col < n_here * D; col += SPLINE_LANES) {
        const int tl = col / D, d = col - tl * D;
        const int base = tl * ND + d;
        ss[base] = 0.0f;
        ss[base + (N - 1) * D] = 0.0f;
        float g = 0.0f;
        for (int i = 1; i < N - 1; ++i) {
            const float b = P.c3 * (ys[base + (i + 1) * D] - ys[base + (i - 1) * D]);
            g = (b - g) * P.piv[i - 1 < SPLINE_PIVOTS - 1 ? i - 1 : SPLINE_PIVOTS - 1];
            ss[base + i * D] = g;
        }
        float s = 0.0f;
        for (int i = N - 2; i >= 1; --i) {
            s = ss[base + i * D] - P.piv[i - 1 < SPLINE_PIVOTS - 1 ? i - 1 : SPLINE_PIVOTS - 1] * s;
            ss[base + i * D] = s;
        }
    }
    __syncthreads();

    const int total = n_here * S * D;
    const int64_t obase = j0 * S * D;
    for (int o = tid; o < total; o += SPLINE_LANES) {
        const int row = o / D, d = o - row * D;
        const int tl = row / S, k = row - tl * S;
        const int i = seg[k];
        const float tau = taus[k];
        const int at = tl * ND + i * D + d;
        const float y0 = ys[at], y1 = ys[at + D], s0 = ss[at], s1 = ss[at + D];
        const float om = 1.0f - tau, dy = y1 - y0;
        const bool end = k == 0 || k == S - 1;
        float p = (y0 + ((tau * tau) * (3.0f - 2.0f * tau)) * dy) + ((P.h * tau) * om) * (om * s0 - tau * s1);
        if (tau == 0.0f) p = y0;                                   // a knot: the input's bits
        if (k == S - 1) p = y1;
        pos[obase + o] = p;
        if (vel) {
            float v = 0.0f;
            if (P.vel_mode == 2) {
                v = (((P.c6 * tau) * om) * dy + (om * (1.0f - 3.0f * tau)) * s0) + (tau * (3.0f * tau - 2.0f)) * s1;
                if (end) v = 0.0f;
            } else if (P.vel_mode == 1) {
                if (!end) v = (ys[tl * ND + D + d] - ys[tl * ND + d]) / P.sdt;
            }
            vel[obase + o] = v;
        }
    }
}

// Way-point variance.  The particles of a (problem, way point) are cut into tiles of 64; a unit is (problem p, way point t, tile pair
// bi <= bj), one wavefront each, four units a workgroup.  Lane l keeps particle bi * 64 + l's position in registers (a) and particle
// bj * 64 + l's (b); for j = 0 .. 63 the position of bj * 64 + j is broadcast from lane j's registers, and the lane adds the
// distance to its own particle if that pair is i < j.  The distance is formed in fp32 from the coordinate differences; the lane's two
// sums, their fold across the wavefront (xor shuffles: a fixed tree) and everything after are fp64.  DMAX in {2, 4, 8, 16, 32} is the
// register room for a position, zero beyond dim; the loops over it are unrolled and the sum over the coordinates is in ascending
// order, so every instantiation gives the same bits.
constexpr int VAR_TILE = 64;

__device__ __forceinline__ float lane_bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// partial [n_problems, n_pairs, horizon, 2] doubles: (S1, S2) of the unit
template <int DMAX>
__global__ void __launch_bounds__(256)
k_waypoint_var_pairs(const float* __restrict__ x, int64_t n_units, int K, int H, int Sd, int c0, int dim, int nb, int n_pairs,
                     double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // the same in every lane of a wavefront
    if (unit >= n_units) return;
    const int64_t pt = unit / n_pairs;
    int u = (int)(unit - pt * n_pairs);
    const int64_t p = pt / H;
    const int t = (int)(pt - p * H);
    const int u_at = u;
    int bi = 0;
    while (u >= nb - bi) { u -= nb - bi; ++bi; }                           // tile pairs in row-major order of the upper triangle
    const int bj = bi + u;
    const int gi = bi * VAR_TILE + lane, gj = bj * VAR_TILE + lane;
    float a[DMAX], b[DMAX];
    const float* const xa = x + ((p * K + (gi < K ? gi : 0)) * H + t) * Sd + c0;
    const float* const xb = x + ((p * K + (gj < K ? gj : 0)) * H + t) * Sd + c0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
        a[d] = 0.0f; b[d] = 0.0f;
        if (d < dim) { a[d] = xa[d]; b[d] = xb[d]; }
    }
    double s1 = 0.0, s2 = 0.0;
    const int jn = K - bj * VAR_TILE < VAR_TILE ? K - bj * VAR_TILE : VAR_TILE;
    for (int j = 0; j < jn; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {                                   // beyond dim both are 0: acc + 0 * 0 is acc, bit for bit
            const float diff = a[d] - lane_bcast(b[d], j);
            acc = acc + diff * diff;
        }
        const float dist = sqrtf(acc);
        if (gi < K && gi < bj * VAR_TILE + j) {
            s1 += (double)dist;
            s2 += (double)dist * (double)dist;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        s1 += __shfl_xor(s1, m);
        s2 += __shfl_xor(s2, m);
    }
    if (lane == 0) {
        double* const out = partial + ((p * n_pairs + u_at) * H + t) * 2;
        out[0] = s1; out[1] = s2;
    }
}

// One workgroup per problem.  Lane l walks the way points t = l, l + 256, ...: the units of a way point in ascending order, then
// var_t = (S2 - S1^2 / n) / (n - 1) with n = K^2, added to the lane's sum in ascending t; the 256 sums fold by a fixed tree in LDS.
__global__ void __launch_bounds__(256)
k_waypoint_var_finish(const double* __restrict__ partial, int K, int H, int n_pairs, float* __restrict__ out) {
    __shared__ double fold[256];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const double n = (double)K * (double)K;
    double sum = 0.0;
    for (int t = tid; t < H; t += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int u = 0; u < n_pairs; ++u) {
            const double* const at = partial + ((p * n_pairs + u) * H + t) * 2;
            s1 += at[0]; s2 += at[1];
        }
        sum += (s2 - s1 * s1 / n) / (n - 1.0);
    }
    fold[tid] = sum;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m) fold[tid] += fold[tid + m];
        __syncthreads();
    }
    if (tid == 0) out[p] = (float)fold[0];
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

int var_tiles(int K) { return (K + VAR_TILE - 1) / VAR_TILE; }
int var_pairs(int K) { const int nb = var_tiles(K); return nb * (nb + 1) / 2; }

// the arguments both variance entries share; 0 = fine
int var_check(const char* who, int64_t n_problems, int32_t n_particles, int32_t horizon) {
    if (n_problems < 0 || n_particles < 1 || horizon < 1)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems >= 0, n_particles >= 1 and horizon >= 1");
    const int64_t most = n_particles > horizon ? n_particles : horizon, least = n_particles > horizon ? horizon : n_particles;
    if (n_problems > 0x3fffffff / most || n_problems * most * least > 0x3fffffff)      // the first bounds the product below 2^60
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * n_particles * horizon above 0x3fffffff");
    return TRK_OK;
}

}  // namespace

extern "C" {

int trk_traj_spline_resample(const float* y, int64_t n_traj, int32_t n_points, int32_t dim, int32_t n_out, int32_t vel_mode, float dt,
                             float* pos, float* vel, trk_stream_t stream) {
    const char* who = "trk_traj_spline_resample";
    if (n_traj < 0 || n_points < 2 || n_out < 2 || dim < 1)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_traj >= 0, n_points >= 2, n_out >= 2 and dim >= 1");
    if (n_traj > 0x3fffffff / (n_points > n_out ? n_points : n_out))
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_traj * max(n_points, n_out) above 0x3fffffff");
    if (vel_mode < 0 || vel_mode > 2) return fail_for(TRK_ERR_INVALID_ARG, who, "vel_mode must be 0 (zero), 1 (average) or 2 (spline)");
    if (vel_mode == 1 && (!std::isfinite(dt) || !(dt > 0.0f))) return fail_for(TRK_ERR_INVALID_ARG, who, "vel_mode 1 needs dt finite and > 0");
    if (vel_mode != 0 && !vel) return fail_for(TRK_ERR_INVALID_ARG, who, "vel_mode 1 and 2 need vel");
    if (n_traj > 0 && (!y || !pos)) return fail_for(TRK_ERR_INVALID_ARG, who, "null y / pos");
    if (n_points > TRK_SPLINE_MAX_POINTS)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "n_points above TRK_SPLINE_MAX_POINTS (256): a workgroup keeps whole trajectories in LDS");
    if (n_out > TRK_SPLINE_MAX_OUT) return fail_for(TRK_ERR_UNSUPPORTED, who, "n_out above TRK_SPLINE_MAX_OUT (1024)");
    if (dim > TRK_SPLINE_MAX_DIM) return fail_for(TRK_ERR_UNSUPPORTED, who, "dim above TRK_SPLINE_MAX_DIM (32)");
    if (n_traj == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    static bool lds_raised = false;                                // the tile (<= 64 KiB) and the sample table (<= 8 KiB)
    if (!lds_raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_spline_resample), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SPLINE_TILE_BYTES + 8 * TRK_SPLINE_MAX_OUT) != hipSuccess)
            return fail_for(TRK_ERR_HIP, who, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        lds_raised = true;
    }
    SplinePar P;
    const double nm1 = (double)(n_points - 1);
    P.h = (float)(1.0 / nm1);
    P.c3 = (float)(3.0 * nm1);
    P.c6 = (float)(6.0 * nm1);
    P.sdt = vel_mode == 1 ? (float)((double)n_out * (double)dt) : 1.0f;
    P.vel_mode = vel_mode;
    double m = 0.25;
    for (int i = 0; i < SPLINE_PIVOTS; ++i) { P.piv[i] = (float)m; m = 1.0 / (4.0 - m); }
    // the tile: what the LDS budget holds, no more than gives every lane a column, and no larger than still fills the chip
    const int traj_bytes = 2 * n_points * dim * (int)sizeof(float);
    int per_wg = SPLINE_TILE_BYTES / traj_bytes;
    const int lanes = (SPLINE_LANES + dim - 1) / dim;
    if (per_wg > lanes) per_wg = lanes;
    const int64_t fill = (n_traj + SPLINE_FILL_GRID - 1) / SPLINE_FILL_GRID;
    if (per_wg > fill) per_wg = (int)fill;
    if (per_wg < 1) per_wg = 1;
    const size_t lds = (size_t)per_wg * traj_bytes + (size_t)n_out * 8;
    const dim3 g((unsigned)((n_traj + per_wg - 1) / per_wg));
    hipLaunchKernelGGL(k_spline_resample, g, dim3(SPLINE_LANES), lds, (hipStream_t)stream, P, y, n_traj, per_wg, n_points, dim, n_out, pos,
                       vel);
    return launched("k_spline_resample");
}

int64_t trk_traj_waypoint_variance_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon) {
    if (n_problems < 0 || n_particles < 1 || n_particles > TRK_WAYPOINT_VAR_MAX_PARTICLES || horizon < 1) return -1;
    return n_problems * (int64_t)var_pairs(n_particles) * horizon * 2 * (int64_t)sizeof(double);
}

int trk_traj_waypoint_variance(const float* x, int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t state_dim, int32_t c0,
                               int32_t dim, float* out, void* workspace, int64_t workspace_bytes, trk_stream_t stream) {
    const char* who = "trk_traj_waypoint_variance";
    if (int rc = var_check(who, n_problems, n_particles, horizon)) return rc;
    if (dim < 1 || c0 < 0 || state_dim < 1 || (int64_t)c0 + dim > state_dim)
        return fail_for(TRK_ERR_INVALID_ARG, who, "dim >= 1, c0 >= 0 and c0 + dim <= state_dim");
    if (n_problems > 0 && (!x || !out)) return fail_for(TRK_ERR_INVALID_ARG, who, "null x / out");
    if (n_particles > TRK_WAYPOINT_VAR_MAX_PARTICLES)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "n_particles above TRK_WAYPOINT_VAR_MAX_PARTICLES (4096)");
    if (dim > TRK_WAYPOINT_VAR_MAX_DIM) return fail_for(TRK_ERR_UNSUPPORTED, who, "dim above TRK_WAYPOINT_VAR_MAX_DIM (32)");
    const int64_t need = trk_traj_waypoint_variance_workspace_bytes(n_problems, n_particles, horizon);
    if (n_problems > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || workspace_bytes < need))
        return fail_for(TRK_ERR_INVALID_ARG, who, "workspace null, not 8-byte aligned or below trk_traj_waypoint_variance_workspace_bytes");
    if (n_problems == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    const int nb = var_tiles(n_particles), n_pairs = var_pairs(n_particles);
    const int64_t n_units = n_problems * horizon * n_pairs;
    hipStream_t st = (hipStream_t)stream;
    double* const partial = static_cast<double*>(workspace);
#define TRK_VAR_PAIRS_GO(DMAX) hipLaunchKernelGGL(k_waypoint_var_pairs<DMAX>, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, st, x, \
                                                  n_units, n_particles, horizon, state_dim, c0, dim, nb, n_pairs, partial)
    if (dim <= 2) TRK_VAR_PAIRS_GO(2);
    else if (dim <= 4) TRK_VAR_PAIRS_GO(4);
    else if (dim <= 8) TRK_VAR_PAIRS_GO(8);
    else if (dim <= 16) TRK_VAR_PAIRS_GO(16);
    else TRK_VAR_PAIRS_GO(32);
#undef TRK_VAR_PAIRS_GO
    if (int rc = launched("k_waypoint_var_pairs")) return rc;
    hipLaunchKernelGGL(k_waypoint_var_finish, dim3((unsigned)n_problems), dim3(256), 0, st, partial, n_particles, horizon, n_pairs, out);
    return launched("k_waypoint_var_finish");
}

}  // extern "C"

// trk_traj_softmin.hip -- the sampling-based trajectory update (include/trk.h, "Sampling-based trajectory update"): the soft-min
// weights of a problem's particles from their costs (trk_traj_softmin_weights: MPPI's per-trajectory weights, STOMP's per-way-point
// probabilities) and the step of the mean towards the weighted particle mean (trk_traj_weighted_update).  Kernels and C entries.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include "trk_launch.h"

namespace {

constexpr int SM_LANES = 1024;                     // one workgroup reduces a problem (or a tile of its way points)
constexpr int SM_TILE_T = 16;                      // way points a workgroup owns in the way-point mode: 64 B of a particle's cost row
constexpr int SM_ONE_LAUNCH = 256;                 // particles up to which the workgroup sums its problem's score rows itself
constexpr int UPD_CHUNK = 64;                      // particles summed in ascending k by one lane
constexpr int UPD_LANES = 64;                      // a wavefront covers 64 consecutive floats of a particle's H * dim row

// a_k of include/trk.h; lo is the candidates' minimum, hi their maximum (the trajectory mode does not look at it)
template <bool WAYPOINT>
__device__ __forceinline__ double softmin_a(double v, double lo, double hi, double lambda) {
    if (WAYPOINT) return hi > lo ? exp(-(v - lo) / ((hi - lo) * lambda)) : 1.0;
    return exp(-(v - lo) / lambda);
}

// S_k = sum_t cost[k, t] of the trajectory mode by G lanes a row (G = the power of two >= min(H, 64), the lanes of one wavefront):
// lane `sub` adds t = sub, sub + G, ... in ascending order, then a xor tree across the G lanes.  Every lane of the wavefront calls it.
__device__ __forceinline__ double row_sum(const float* __restrict__ at, bool on, int H, int G, int sub) {
    double sum = 0.0;
    if (on)
        for (int i = sub; i < H; i += G) sum += (double)at[i];
    for (int m = G >> 1; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    return sum;
}

// More than SM_ONE_LAUNCH particles: the rows of all problems are summed across the chip first, 256 / G rows a workgroup, into
// S [n_problems * K] doubles (NaN for a rejected particle) -- the same arithmetic as inside k_softmin_weights, so the same bits.
__global__ void __launch_bounds__(256)
k_softmin_row_sums(const float* __restrict__ cost, const uint8_t* __restrict__ valid, int64_t n_rows, int H, int G, double* __restrict__ S) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool on = row < n_rows;
    const double sum = row_sum(cost + (on ? row : 0) * H, on, H, G, sub);
    if (on && sub == 0) S[row] = (valid && valid[row] == 0) ? __builtin_nan("") : sum;
}

// One workgroup per (problem, tile): the trajectory mode has one tile and one column (TW = 1), the way-point mode tiles of TW = 16
// way points.  Lane (c, g) = (tid % TW, tid / TW) walks the particles k = g, g + NG, ... of column c three times -- the candidates'
// min and max, the sums Z and sum a^2 (ascending k, then a fixed tree over g in LDS), the weights -- so the association depends
// on K alone.  A score that is not a candidate's is carried as NaN.  Trajectory mode, first: S_k = sum_t cost[k, t] by G lanes a
// particle (row_sum), or read from S_in where k_softmin_row_sums has run; S_k stays in LDS.  Every lane reaches every barrier: a lane beyond H or K only has nothing to add.
template <bool WAYPOINT>
__global__ void __launch_bounds__(SM_LANES)
k_softmin_weights(const float* __restrict__ cost, const uint8_t* __restrict__ valid, int K, int H, int G, double lambda, int tiles,
                  const double* __restrict__ S_in, float* __restrict__ w, float* __restrict__ ess) {
    constexpr int TW = WAYPOINT ? SM_TILE_T : 1;
    constexpr int NG = SM_LANES / TW;
    __shared__ double fold_a[SM_LANES], fold_b[SM_LANES];
    __shared__ double S[WAYPOINT ? 1 : TRK_SOFTMIN_MAX_PARTICLES];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - p * tiles);
    const int c = tid % TW, g = tid / TW;
    const int t = tile * TW + c;
    const bool live = t < H;
    const int64_t row0 = p * K;
    const double nan = __builtin_nan("");

    if (!WAYPOINT) {
        if (S_in) {
            for (int k = tid; k < K; k += SM_LANES) S[k] = S_in[row0 + k];
        } else {
            const int sub = tid & (G - 1), slot = tid / G, per_pass = SM_LANES / G;
            for (int k0 = 0; k0 < K; k0 += per_pass) {
                const int k = k0 + slot;
                const double sum = row_sum(cost + (row0 + (k < K ? k : 0)) * H, k < K, H, G, sub);
                if (k < K && sub == 0) S[k] = (valid && valid[row0 + k] == 0) ? nan : sum;
            }
        }
        __syncthreads();
    }
    auto value = [&](int k) -> double {
        if (!WAYPOINT) return S[k];
        if (!live || (valid && valid[row0 + k] == 0)) return nan;
        return (double)cost[(row0 + k) * H + t];
    };

    double lo = INFINITY, hi = -INFINITY;
    for (int k = g; k < K; k += NG) {
        const double v = value(k);
        if (__builtin_isfinite(v)) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    }
    fold_a[tid] = lo; fold_b[tid] = hi;
    __syncthreads();
    for (int m = NG >> 1; m >= 1; m >>= 1) {
        if (g < m) {
            const double a = fold_a[tid + m * TW], b = fold_b[tid + m * TW];
            if (a < fold_a[tid]) fold_a[tid] = a;
            if (b > fold_b[tid]) fold_b[tid] = b;
        }
        __syncthreads();
    }
    lo = fold_a[c]; hi = fold_b[c];
    __syncthreads();

    double z = 0.0, z2 = 0.0;
    for (int k = g; k < K; k += NG) {
        const double v = value(k);
        if (__builtin_isfinite(v)) {
            const double a = softmin_a<WAYPOINT>(v, lo, hi, lambda);
            z += a; z2 += a * a;
        }
    }
    fold_a[tid] = z; fold_b[tid] = z2;
    __syncthreads();
    for (int m = NG >> 1; m >= 1; m >>= 1) {
        if (g < m) { fold_a[tid] += fold_a[tid + m * TW]; fold_b[tid] += fold_b[tid + m * TW]; }
        __syncthreads();
    }
    z = fold_a[c]; z2 = fold_b[c];

    if (live) {
        for (int k = g; k < K; k += NG) {
            const double v = value(k);
            float wk = 0.0f;
            if (__builtin_isfinite(v)) wk = (float)(softmin_a<WAYPOINT>(v, lo, hi, lambda) / z);
            w[WAYPOINT ? (row0 + k) * H + t : row0 + k] = wk;
        }
        if (g == 0 && ess) ess[WAYPOINT ? p * H + t : p] = lo <= hi ? (float)(z * z / z2) : 0.0f;
    }
}

// out = mean + step * acc of include/trk.h, the pins and the clamp; t, d: the element's way point and coordinate
__device__ __forceinline__ float update_finish(float m, float acc, float step, int pin, int t, int H, const float* __restrict__ lo,
                                               const float* __restrict__ hi, int d) {
    const bool pinned = (t == 0 && (pin & 1)) || (t == H - 1 && (pin & 2));
    float r = m + step * acc;
    if (step == 0.0f) r = m;
    if (lo && !pinned) {
        const float l = lo[d], h = hi[d];
        r = r < l ? l : r;
        r = r > h ? h : r;
    }
    return pinned ? m : r;
}

// A workgroup is one wavefront: the unit (problem p, chunk of 64 particles, tile of 64 elements e of the H * dim row).  The lane adds
// w_k (x_k - mean) of its element over the chunk's particles in ascending k; a weight of exactly 0 leaves the sum by a select.  FINAL
// (K <= 64, one chunk): the lane finishes the element.  Otherwise the chunk's sum goes to partial [n_problems, n_chunks, E].
template <bool FINAL>
__global__ void __launch_bounds__(UPD_LANES)
k_weighted_update(const float* __restrict__ x, const float* mean, const float* __restrict__ w, const float* __restrict__ lo,
                  const float* __restrict__ hi, int K, int H, int D, int64_t E, int e_tiles, int n_chunks, float step, int pin, int per_wp,
                  float* out) {
    const int64_t unit = blockIdx.x;
    const int e_tile = (int)(unit % e_tiles);
    const int64_t rest = unit / e_tiles;
    const int chunk = (int)(rest % n_chunks);
    const int64_t p = rest / n_chunks;
    const int64_t e = (int64_t)e_tile * UPD_LANES + threadIdx.x;
    if (e >= E) return;
    const int t = (int)(e / D), d = (int)(e - (int64_t)t * D);
    const float m = mean[p * E + e];
    const int k0 = chunk * UPD_CHUNK;
    const int kn = K - k0 < UPD_CHUNK ? K - k0 : UPD_CHUNK;
    const int64_t row0 = p * K + k0;
    float acc = 0.0f;
#pragma unroll 8
    for (int k = 0; k < kn; ++k) {
        const int64_t row = row0 + k;
        const float wk = w[per_wp ? row * H + t : row];
        const float dx = x[row * E + e] - m;
        const float s = acc + wk * dx;
        acc = wk != 0.0f ? s : acc;
    }
    if (FINAL) out[p * E + e] = update_finish(m, acc, step, pin, t, H, lo, hi, d);
    else out[(p * n_chunks + chunk) * E + e] = acc;
}

// K > 64: one lane per element adds the chunks' sums in ascending chunk order and finishes the element
__global__ void __launch_bounds__(256)
k_weighted_update_finish(const float* __restrict__ partial, const float* mean, const float* __restrict__ lo, const float* __restrict__ hi,
                         int H, int D, int64_t E, int e_tiles, int n_chunks, float step, int pin, float* out) {
    const int64_t p = blockIdx.x / e_tiles;
    const int64_t e = (int64_t)(blockIdx.x - p * e_tiles) * 256 + threadIdx.x;
    if (e >= E) return;
    const int t = (int)(e / D), d = (int)(e - (int64_t)t * D);
    const float* const at = partial + p * n_chunks * E + e;
    float acc = at[0];
    for (int j = 1; j < n_chunks; ++j) acc = acc + at[j * E];
    out[p * E + e] = update_finish(mean[p * E + e], acc, step, pin, t, H, lo, hi, d);
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

int update_chunks(int K) { return (K + UPD_CHUNK - 1) / UPD_CHUNK; }

}  // namespace

extern "C" {

int64_t trk_traj_softmin_weights_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t mode) {
    if (n_problems < 0 || n_particles < 1 || n_particles > TRK_SOFTMIN_MAX_PARTICLES || horizon < 1) return -1;
    if ((mode != TRK_SOFTMIN_TRAJECTORY && mode != TRK_SOFTMIN_WAYPOINT) || n_problems > 0x3fffffff / n_particles) return -1;
    if (mode == TRK_SOFTMIN_WAYPOINT || horizon == 1 || n_particles <= SM_ONE_LAUNCH) return 0;
    return n_problems * n_particles * (int64_t)sizeof(double);
}

int trk_traj_softmin_weights(const TrkSoftmin* s, const float* cost, const uint8_t* valid, int64_t n_problems, int32_t horizon, float* w,
                             float* ess, void* workspace, int64_t workspace_bytes, trk_stream_t stream) {
    const char* who = "trk_traj_softmin_weights";
    if (!s) return fail_for(TRK_ERR_INVALID_ARG, who, "null s");
    if (!std::isfinite(s->temperature) || !(s->temperature > 0.0f))
        return fail_for(TRK_ERR_INVALID_ARG, who, "temperature must be finite and > 0");
    if (s->mode != TRK_SOFTMIN_TRAJECTORY && s->mode != TRK_SOFTMIN_WAYPOINT)
        return fail_for(TRK_ERR_INVALID_ARG, who, "mode must be TRK_SOFTMIN_TRAJECTORY (0) or TRK_SOFTMIN_WAYPOINT (1)");
    if (n_problems < 0 || s->n_particles < 1 || horizon < 1)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems >= 0, n_particles >= 1 and horizon >= 1");
    if (n_problems > 0x3fffffff / s->n_particles) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * n_particles above 0x3fffffff");
    const int64_t tiles = s->mode == TRK_SOFTMIN_WAYPOINT ? ((int64_t)horizon + SM_TILE_T - 1) / SM_TILE_T : 1;
    if (n_problems > 0x7fffffff / tiles) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * ceil(horizon / 16) above 0x7fffffff");
    if (n_problems > 0 && (!cost || !w)) return fail_for(TRK_ERR_INVALID_ARG, who, "null cost / w");
    if (s->n_particles > TRK_SOFTMIN_MAX_PARTICLES)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "n_particles above TRK_SOFTMIN_MAX_PARTICLES (4096): a workgroup keeps a problem's scores in LDS");
    const int64_t need = trk_traj_softmin_weights_workspace_bytes(n_problems, s->n_particles, horizon, s->mode);
    if (n_problems > 0 && need > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || workspace_bytes < need))
        return fail_for(TRK_ERR_INVALID_ARG, who, "workspace null, not 8-byte aligned or below trk_traj_softmin_weights_workspace_bytes");
    if (n_problems == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    const double lambda = (double)s->temperature;
    const dim3 grid((unsigned)(n_problems * tiles));
    if (s->mode == TRK_SOFTMIN_WAYPOINT) {
        hipLaunchKernelGGL(k_softmin_weights<true>, grid, dim3(SM_LANES), 0, (hipStream_t)stream, cost, valid, s->n_particles, horizon, 1,
                           lambda, (int)tiles, static_cast<const double*>(nullptr), w, ess);
    } else {
        int G = 1;
        while (G < 64 && G < horizon) G <<= 1;
        const double* S = nullptr;
        if (need > 0) {
            const int64_t n_rows = n_problems * s->n_particles;
            const int per_wg = 256 / G;
            hipLaunchKernelGGL(k_softmin_row_sums, dim3((unsigned)((n_rows + per_wg - 1) / per_wg)), dim3(256), 0, (hipStream_t)stream, cost,
                               valid, n_rows, horizon, G, static_cast<double*>(workspace));
            if (int rc = launched("k_softmin_row_sums")) return rc;
            S = static_cast<const double*>(workspace);
        }
        hipLaunchKernelGGL(k_softmin_weights<false>, grid, dim3(SM_LANES), 0, (hipStream_t)stream, cost, valid, s->n_particles, horizon, G,
                           lambda, 1, S, w, ess);
    }
    return launched("k_softmin_weights");
}

int64_t trk_traj_weighted_update_workspace_bytes(int64_t n_problems, int32_t n_particles, int32_t horizon, int32_t dim) {
    if (n_problems < 0 || n_particles < 1 || n_particles > TRK_SOFTMIN_MAX_PARTICLES || horizon < 1 || dim < 1) return -1;
    if ((int64_t)horizon * dim > 0x3fffffff || n_problems > 0x3fffffff / n_particles) return -1;
    if (n_particles <= UPD_CHUNK) return 0;
    return n_problems * update_chunks(n_particles) * (int64_t)horizon * dim * (int64_t)sizeof(float);
}

int trk_traj_weighted_update(const TrkWeightedUpdate* u, const float* x, const float* mean, const float* w, const float* lo, const float* hi,
                             int64_t n_problems, int32_t horizon, int32_t dim, float* out, void* workspace, int64_t workspace_bytes,
                             trk_stream_t stream) {
    const char* who = "trk_traj_weighted_update";
    if (!u) return fail_for(TRK_ERR_INVALID_ARG, who, "null u");
    if (!std::isfinite(u->step)) return fail_for(TRK_ERR_INVALID_ARG, who, "step must be finite");
    if (u->pin < 0 || u->pin > 3) return fail_for(TRK_ERR_INVALID_ARG, who, "pin must be 0 .. 3 (bit 0: the first way point, bit 1: the last)");
    if (u->w_per_waypoint != 0 && u->w_per_waypoint != 1) return fail_for(TRK_ERR_INVALID_ARG, who, "w_per_waypoint must be 0 or 1");
    if (n_problems < 0 || u->n_particles < 1 || horizon < 1 || dim < 1)
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems >= 0, n_particles >= 1, horizon >= 1 and dim >= 1");
    if (n_problems > 0x3fffffff / u->n_particles) return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * n_particles above 0x3fffffff");
    const int64_t E = (int64_t)horizon * dim;
    if (E > 0x3fffffff) return fail_for(TRK_ERR_INVALID_ARG, who, "horizon * dim above 0x3fffffff");
    if ((lo == nullptr) != (hi == nullptr)) return fail_for(TRK_ERR_INVALID_ARG, who, "lo and hi come together (only one of lo / hi given)");
    if (n_problems > 0 && (!x || !mean || !w || !out)) return fail_for(TRK_ERR_INVALID_ARG, who, "null x / mean / w / out");
    if (u->n_particles > TRK_SOFTMIN_MAX_PARTICLES)
        return fail_for(TRK_ERR_UNSUPPORTED, who, "n_particles above TRK_SOFTMIN_MAX_PARTICLES (4096)");
    const int n_chunks = update_chunks(u->n_particles);
    const int64_t e_tiles = (E + UPD_LANES - 1) / UPD_LANES;
    if (n_problems > 0x7fffffff / (e_tiles * n_chunks))
        return fail_for(TRK_ERR_INVALID_ARG, who, "n_problems * ceil(n_particles / 64) * ceil(horizon * dim / 64) above 0x7fffffff");
    const int64_t need = trk_traj_weighted_update_workspace_bytes(n_problems, u->n_particles, horizon, dim);
    if (n_problems > 0 && need > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3) != 0 || workspace_bytes < need))
        return fail_for(TRK_ERR_INVALID_ARG, who, "workspace null, not 4-byte aligned or below trk_traj_weighted_update_workspace_bytes");
    if (n_problems == 0) return TRK_OK;
    if (int rc = trk_ensure_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_problems * n_chunks * e_tiles));
    if (n_chunks == 1) {
        hipLaunchKernelGGL(k_weighted_update<true>, grid, dim3(UPD_LANES), 0, st, x, mean, w, lo, hi, u->n_particles, horizon, dim, E,
                           (int)e_tiles, 1, u->step, u->pin, u->w_per_waypoint, out);
        return launched("k_weighted_update");
    }
    float* const partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_weighted_update<false>, grid, dim3(UPD_LANES), 0, st, x, mean, w, lo, hi, u->n_particles, horizon, dim, E,
                       (int)e_tiles, n_chunks, u->step, u->pin, u->w_per_waypoint, partial);
    if (int rc = launched("k_weighted_update")) return rc;
    const int64_t f_tiles = (E + 255) / 256;
    hipLaunchKernelGGL(k_weighted_update_finish, dim3((unsigned)(n_problems * f_tiles)), dim3(256), 0, st, partial, mean, lo, hi, horizon, dim,
                       E, (int)f_tiles, n_chunks, u->step, u->pin, out);
    return launched("k_weighted_update_finish");
}

}  // extern "C"

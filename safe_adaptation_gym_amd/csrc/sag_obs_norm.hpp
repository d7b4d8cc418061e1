// sag_obs_norm.hpp - observation normalisation on the context stream (include/sag.h defines the three functions):
//   k_obs_partial<PASS>   one [obs_dim] fp32 partial per block over chunks of OBSN_CHUNK logical rows
//                         PASS 0: column sums of x   1: column sums of (x - s)^2, s = the fp32 batch mean of pass 0
//   k_obs_mean            the pass-0 partials added in ascending block order in fp64 -> the batch mean and its fp32 rounding
//   k_obs_merge           the pass-1 partials likewise -> the batch M2, merged into the caller's fp64 state (Chan et al.), then
//                         the table; with table_only it rewrites the table from the state and reads nothing else
//   obs_norm_piece        what the policy kernels apply to a staged 16-byte piece (sag_policy.hpp, sag_policy_grad.hpp)
// Logical row e (0 <= e < n_planes * n_rows) is row e % n_rows of plane e / n_rows, at float offset
// (plane * pitch + row) * obs_pitch.  With Q = obs_dim / 4 pieces of 16 bytes per row a block takes R = 256 / Q rows per round:
// thread t < R Q holds piece t % Q of row t / Q, so its four columns never change and their accumulators stay in registers;
// a round is one coalesced 16-byte load per thread and OBSN_FLIGHT rounds are in flight before the first add.  At the end the R
// threads of a column quad are added through LDS in ascending row order.  Pad rows and pad columns are never loaded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sag {

constexpr int OBSN_THREADS = 256;
constexpr int OBSN_CHUNK = 1024;        // logical rows: a block's unit of work
constexpr int OBSN_FLIGHT = 4;          // rounds (16-byte loads per thread) in flight
constexpr int OBSN_MAX_BLOCKS = 1024;   // the default cap too
constexpr int OBSN_MAX_OBS = 104;

// the grid: a function of the number of rows and max_blocks only
inline int obsn_grid(int64_t rows, int max_blocks) {
  const int64_t chunks = (rows + OBSN_CHUNK - 1) / OBSN_CHUNK;
  const int64_t cap = max_blocks > 0 ? (max_blocks < OBSN_MAX_BLOCKS ? max_blocks : OBSN_MAX_BLOCKS) : OBSN_MAX_BLOCKS;
  return (int)(chunks < cap ? chunks : cap);
}

// the workspace: [OBSN_MAX_OBS] f64 batch means, [OBSN_MAX_OBS] f32 roundings of them, then [grid][obs_dim] f32 partials
inline size_t obsn_ws_bytes(int grid, int obs_dim) { return (size_t)OBSN_MAX_OBS * 12 + (size_t)grid * obs_dim * sizeof(float); }

// xh = fl(fl(x - mean) * rstd) clamped to [-clip, clip]; a NaN passes both comparisons
__device__ inline float obs_norm_one(float x, float m, float r, float clip) {
#pragma clang fp contract(off)
  const float d = x - m;
  float xh = d * r;
  xh = xh < -clip ? -clip : xh;
  xh = xh > clip ? clip : xh;
  return xh;
}

// piece q (columns 4 q ... 4 q + 3) of a row under table = mean [obs_dim] then rstd [obs_dim]
__device__ inline float4 obs_norm_piece(float4 v, const float* table, int obs_dim, int q, float clip) {
  const float4 m = *reinterpret_cast<const float4*>(table + 4 * q);
  const float4 r = *reinterpret_cast<const float4*>(table + obs_dim + 4 * q);
  return make_float4(obs_norm_one(v.x, m.x, r.x, clip), obs_norm_one(v.y, m.y, r.y, clip), obs_norm_one(v.z, m.z, r.z, clip),
                     obs_norm_one(v.w, m.w, r.w, clip));
}

struct ObsStatsArgs {
  uint32_t total, n_rows, pitch, obs_pitch;   // total = n_planes * n_rows < 2^31
  int32_t obs_dim;
  const float* obs;
  const float* shift;   // PASS 1: [obs_dim] fp32 batch means
  float* part;          // [gridDim.x][obs_dim]
};

template <int PASS>
__global__ __launch_bounds__(OBSN_THREADS) void k_obs_partial(ObsStatsArgs a) {
#pragma clang fp contract(off)
  __shared__ float4 red[OBSN_THREADS];
  const int tid = threadIdx.x;
  const int Q = a.obs_dim >> 2, R = OBSN_THREADS / Q;
  const int rr = tid / Q, q = tid - rr * Q;
  const bool live = rr < R;   // the last 256 - R Q threads hold no piece
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (PASS == 1 && live) s = *reinterpret_cast<const float4*>(a.shift + 4 * q);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t chunks = (a.total + OBSN_CHUNK - 1) / OBSN_CHUNK;
  for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint32_t e0 = c * (uint32_t)OBSN_CHUNK;
    const uint32_t e1 = a.total - e0 < (uint32_t)OBSN_CHUNK ? a.total : e0 + OBSN_CHUNK;
    for (uint32_t base = e0; base < e1; base += (uint32_t)(OBSN_FLIGHT * R)) {
      float4 v[OBSN_FLIGHT];
      bool ok[OBSN_FLIGHT];
#pragma unroll
      for (int j = 0; j < OBSN_FLIGHT; j++) {
        const uint32_t e = base + (uint32_t)(j * R + rr);
        ok[j] = live && e < e1;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[j]) {
          size_t src = e;
          if (a.pitch != a.n_rows) {
            const uint32_t p = e / a.n_rows;
            src = (size_t)p * a.pitch + (e - p * a.n_rows);
          }
          v[j] = *reinterpret_cast<const float4*>(a.obs + src * (size_t)a.obs_pitch + 4 * q);
        }
      }
#pragma unroll
      for (int j = 0; j < OBSN_FLIGHT; j++)
        if (ok[j]) {
          if (PASS == 0) {
            acc.x = acc.x + v[j].x; acc.y = acc.y + v[j].y; acc.z = acc.z + v[j].z; acc.w = acc.w + v[j].w;
          } else {
            const float dx = v[j].x - s.x, dy = v[j].y - s.y, dz = v[j].z - s.z, dw = v[j].w - s.w;
            const float qx = dx * dx, qy = dy * dy, qz = dz * dz, qw = dw * dw;
            acc.x = acc.x + qx; acc.y = acc.y + qy; acc.z = acc.z + qz; acc.w = acc.w + qw;
          }
        }
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < Q) {   // the R rows of this column quad, ascending
    float4 t = red[tid];
    for (int r = 1; r < R; r++) {
      const float4 o = red[r * Q + tid];
      t.x = t.x + o.x; t.y = t.y + o.y; t.z = t.z + o.z; t.w = t.w + o.w;
    }
    *reinterpret_cast<float4*>(a.part + (size_t)blockIdx.x * a.obs_dim + 4 * tid) = t;
  }
}

// column k of the partials in ascending block order, in fp64
__device__ inline double obsn_add_partials(const float* part, int n_blocks, int obs_dim, int k) {
#pragma clang fp contract(off)
  double t = 0.0;
  for (int b = 0; b < n_blocks; b++) t = t + (double)part[(size_t)b * obs_dim + k];
  return t;
}

// mean_b = sum / n_b, shift = (float)mean_b
__global__ __launch_bounds__(OBSN_THREADS) void k_obs_mean(const float* part, int n_blocks, int obs_dim, double n_b, double* mean_b, float* shift) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  if (k >= obs_dim) return;
  const double m = obsn_add_partials(part, n_blocks, obs_dim, k) / n_b;
  mean_b[k] = m;
  shift[k] = (float)m;
}

struct ObsMergeArgs {
  int32_t n_blocks, obs_dim, table_only;
  float eps;
  double n_b;
  const float* part; const double* mean_b; const float* shift;
  double* state;   // {count, mean [obs_dim], M2 [obs_dim]}
  float* table;    // mean [obs_dim], rstd [obs_dim]
};

__global__ __launch_bounds__(OBSN_THREADS) void k_obs_merge(ObsMergeArgs a) {
#pragma clang fp contract(off)
  const int k = threadIdx.x, od = a.obs_dim;
  const double n_a = a.state[0];
  __syncthreads();   // every thread has read the count before thread 0 replaces it
  if (k >= od) return;
  double n = n_a, mean = a.state[1 + k], M2 = a.state[1 + od + k];
  if (!a.table_only) {
    const double sum = obsn_add_partials(a.part, a.n_blocks, od, k);
    const double mean_b = a.mean_b[k], n_b = a.n_b;
    const double ds = mean_b - (double)a.shift[k];
    const double corr = n_b * (ds * ds);
    const double m2 = sum - corr;
    const double M2_b = m2 > 0.0 ? m2 : 0.0;
    n = n_a + n_b;
    const double w = n_b / n;                 // 1 exactly on an empty state
    const double delta = mean_b - mean;
    mean = mean + delta * w;
    M2 = (M2 + M2_b) + (delta * delta) * (n_a * w);
    a.state[1 + k] = mean;
    a.state[1 + od + k] = M2;
    if (k == 0) a.state[0] = n;
  }
  if (n > 0.0) {
    const double var = M2 / n;
    const double den = sqrt(var + (double)a.eps);
    a.table[k] = (float)mean;
    a.table[od + k] = (float)(1.0 / den);
  } else {
    a.table[k] = 0.0f;
    a.table[od + k] = 1.0f;
  }
}

}  // namespace sag

// sag_policy_grad.hpp - the learner's update on the context stream (include/sag.h defines both functions):
//   k_policy_backward<NT>   the gradient of the PPO-Lagrangian loss through the MLP of sag_policy.hpp, hidden = 32 * NT <= 128:
//                           persistent blocks of four wavefronts, one partial [n_params + 8] per block, no atomics
//                           (k_policy_backward<NT, true>: over observations normalised where they are staged,
//                           sag_policy_backward_norm_device; k_policy_backward<NT, NORM, true>: over a list of rows gathered
//                           where they are staged, sag_policy_backward_rows_device)
//   k_policy_grad_reduce    the partials summed in ascending block order into d_grad
//   k_adam                  the elementwise optimiser step
// Per tile of 32 rows a block keeps four images in LDS, all [row][unit] at a pitch of 4 (mod 32) floats: X (the staged
// observations, padded with zeros to a multiple of 32 columns), I1 (h1, later dz1 in place), I2 (h2, later dz2 in place) and DO
// (the head outputs, then the head gradient with the per-row std terms and statistics behind it).  Every product runs on
// pol_mfma and its output tiles of 32 units are dealt round-robin to the four wavefronts:
//   forward     D^T = W^T X^T as in k_policy_forward: A = W[k][unit] from global memory, B = image[row][k], k = 2 s + half in
//               ascending order from the bias, so the chain is the forward's bit for bit and relu' = (h > 0) is its own mask.
//               Units keep natural labels here: register r of lane half h is unit (r & 3) + 8 (r >> 2) + 4 h, four consecutive
//               units per register quad, stored to the image as one 16-byte piece.
//   backward    dh^T = W dz^T: A = W[unit][j] (a lane walks its own weight row: k-steps 4 q ... 4 q + 3 of half h are
//               j = 8 q + 4 h ... + 3, four consecutive floats), B = dz image[row][j] as one 16-byte LDS read.
//   dW          act^T dz over the tile's rows: A = act image[row][in unit], B = dz image[row][out unit], row = 2 s + half; both
//               reads are 32 consecutive floats per half.  The accumulators live in registers across the block's whole loop.
// Biases, the std gradient and the statistics are column sums of the images, one (or two) columns per thread, rows ascending.
#pragma once
#include "sag_policy.hpp"

namespace sag {

constexpr int PGRAD_WAVES = 4;
constexpr int PGRAD_THREADS = PGRAD_WAVES * WAVE;
constexpr int PGRAD_MAX_TILES = 4;          // hidden <= 128: beyond it the dW accumulators of a wavefront do not fit its registers
constexpr int PGRAD_DO_PITCH = 40;          // DO columns: 0 ... 15 dO (nu + 2 used), 16 ... 27 d/dstd per row, 28 ... 35 statistics
constexpr int PGRAD_DO_STD = 16, PGRAD_DO_STAT = 28;
constexpr int PGRAD_STATS = 8;
constexpr int PGRAD_DEFAULT_BLOCKS = 256;   // one per CU of an MI355X
constexpr int PGRAD_MAX_BLOCKS = 1024;

inline int pgrad_x_pitch(int obs_dim) { return 32 * ((obs_dim + 31) / 32) + 4; }
inline size_t pgrad_lds_floats(int obs_dim, int hidden) { return (size_t)POLICY_ROWS * (pgrad_x_pitch(obs_dim) + 2 * (hidden + 4) + PGRAD_DO_PITCH); }
// the grid: a function of the number of rows and max_blocks only
inline int pgrad_grid(int64_t rows, int max_blocks) {
  const int64_t tiles = (rows + POLICY_ROWS - 1) / POLICY_ROWS;
  const int64_t cap = max_blocks > 0 ? (max_blocks < PGRAD_MAX_BLOCKS ? max_blocks : PGRAD_MAX_BLOCKS) : PGRAD_DEFAULT_BLOCKS;
  return (int)(tiles < cap ? tiles : cap);
}

struct PolicyGradArgs {
  int64_t total;   // n_planes * n_rows
  int32_t n_rows, pitch, obs_dim, nu, activation, obs_pitch, n_params;
  float clip, vf, cvf, ent, adv_mul, adv_sub, cadv_mul, cadv_sub;
  const float* params;
  const float* obs; const float* actions; const float* logp_old; const float* adv; const float* ret;
  const float* cadv; const float* cret;
  float* part;   // [gridDim.x][n_params + 8]
};
// sag_policy_backward_norm_device: the same, with every staged observation element normalised under `table`
struct PolicyGradNormArgs : PolicyGradArgs {
  const float* table;   // mean [obs_dim], rstd [obs_dim]
  float obs_clip;
};
// sag_policy_backward_rows_device: `total` is the length of the row list, `limit` = n_planes * n_rows what an entry must be below
struct PolicyGradRowsArgs : PolicyGradNormArgs {
  const int32_t* rows;
  int64_t limit;
};
constexpr int PGRAD_ROWS_LDS_FLOATS = 2 * POLICY_ROWS;   // the ROWS instances' 32 source rows, int64, behind the four images

// Between two output tiles the compiler must not hoist the next tile's 32 LDS reads above this tile's MFMAs: with nine tiles
// unrolled it otherwise keeps hundreds of loaded operands live and spills the accumulators.
#if SAG_HOSTEMU
#define PGRAD_TILE_FENCE() ((void)0)
#else
#define PGRAD_TILE_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

__device__ inline int pgrad_rho(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// act'(z) from h = act(z): relu z > 0 <=> h > 0; tanh 1 - h^2
__device__ inline float pgrad_dact(float h, int activation) {
  if (activation == 0) return h > 0.0f ? 1.0f : 0.0f;
  return 1.0f - h * h;
}

// one output tile of a forward layer: units 32 m ... + 31 of W [K][ldw] (units at or beyond n_units are zero rows)
__device__ inline pol_acc pgrad_forward_tile(const float* W, const float* b, int ldw, int n_units, int K, const float* in, int PI, int m,
                                             int col, int half) {
  pol_acc acc;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int u = 32 * m + pgrad_rho(r, half);
    acc[r] = u < n_units ? b[u] : 0.0f;
  }
  const int u = 32 * m + col;
  const bool ok = u < n_units;
  const float* w = W + (ok ? u : 0);
  const float* x = in + col * PI;
#pragma unroll 8
  for (int s = 0; s < (K >> 1); s++) {
    const int k = 2 * s + half;
    const float a = ok ? w[(size_t)k * ldw] : 0.0f;
    acc = pol_mfma(a, x[k], acc);
  }
  PGRAD_TILE_FENCE();
  return acc;
}

// register quads 4 g ... 4 g + 3 of a result tile are units 32 m + 8 g + 4 half ... + 3 of row `col`
__device__ inline void pgrad_store_tile(float* img, int P, int m, const pol_acc& acc, int col, int half) {
#pragma unroll
  for (int g = 0; g < 4; g++)
    *reinterpret_cast<float4*>(img + col * P + 32 * m + 8 * g + 4 * half) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
}

// dz = dh * act'(h), written over h: a lane reads and writes the same four floats
__device__ inline void pgrad_store_dz(float* img, int P, int m, const pol_acc& dh, int col, int half, int activation) {
#pragma unroll
  for (int g = 0; g < 4; g++) {
    float4* q = reinterpret_cast<float4*>(img + col * P + 32 * m + 8 * g + 4 * half);
    const float4 h = *q;
    *q = make_float4(dh[4 * g] * pgrad_dact(h.x, activation), dh[4 * g + 1] * pgrad_dact(h.y, activation),
                     dh[4 * g + 2] * pgrad_dact(h.z, activation), dh[4 * g + 3] * pgrad_dact(h.w, activation));
  }
}

// dW tile += A image[row][ca + lane unit] * B image[row][cb + lane unit] over the 32 rows
__device__ inline pol_acc pgrad_dw_tile(pol_acc acc, const float* A, int PA, int ca, const float* B, int PB, int cb, int col, int half) {
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const int row = 2 * s + half;
    acc = pol_mfma(A[row * PA + ca + col], B[row * PB + cb + col], acc);
  }
  PGRAD_TILE_FENCE();
  return acc;
}

// register r of lane (col, half) is dW[32 ki + rho][32 mj + col]
__device__ inline void pgrad_put_tile(float* out, int ld, int K, int J, int ki, int mj, const pol_acc& acc, int col, int half) {
  const int c = 32 * mj + col;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int i = 32 * ki + pgrad_rho(r, half);
    if (i < K && c < J) out[(size_t)i * ld + c] = acc[r];
  }
}

template <bool NORM, bool ROWS = false> struct PolicyGradArgsOf { typedef PolicyGradArgs type; };
template <> struct PolicyGradArgsOf<true, false> { typedef PolicyGradNormArgs type; };
template <bool NORM> struct PolicyGradArgsOf<NORM, true> { typedef PolicyGradRowsArgs type; };

// NORM: sag_policy_backward_norm_device; the plain instances are what they were before the switch existed
// ROWS: sag_policy_backward_rows_device - batch row j is logical element rows[j] of the planes.  A tile's 32 entries are turned
//       into source rows once, into 32 words of LDS behind the images (-1: absent - at or beyond the list's end, or an entry
//       outside the planes), and the staging loop and the head lane both take `src` from there.  Everything else is the code of
//       the contiguous instances, which the switch leaves what they were.
template <int NT, bool NORM = false, bool ROWS = false>
__global__ __launch_bounds__(PGRAD_THREADS) void k_policy_backward(typename PolicyGradArgsOf<NORM, ROWS>::type p) {
#pragma clang fp contract(off)
  constexpr int H = 32 * NT, PH = H + 4, PD = PGRAD_DO_PITCH;
  constexpr int T3 = (NT + PGRAD_WAVES - 1) / PGRAD_WAVES, T2 = (NT * NT + PGRAD_WAVES - 1) / PGRAD_WAVES, T1 = NT;   // tiles per wavefront
  HIP_DYNAMIC_SHARED(float4, lds4)
  float* lds = reinterpret_cast<float*>(lds4);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int od = p.obs_dim, nu = p.nu, NO = nu + 2, Q = od >> 2;
  const int KT1 = (od + 31) >> 5, PX = 32 * KT1 + 4;
  float* X = lds;
  float* I1 = X + POLICY_ROWS * PX;
  float* I2 = I1 + POLICY_ROWS * PH;
  float* DO = I2 + POLICY_ROWS * PH;
  const int lds_floats = POLICY_ROWS * (PX + 2 * PH + PD);
  for (int k = tid; k < lds_floats; k += PGRAD_THREADS) lds[k] = 0.0f;   // the pad columns of X stay zero
  int64_t* SRC = reinterpret_cast<int64_t*>(lds + lds_floats);   // ROWS only (lds_floats is a multiple of 32: aligned)
  (void)SRC;

  const float* W1 = p.params;
  const float* b1 = W1 + (size_t)od * H;
  const float* W2 = b1 + H;
  const float* b2 = W2 + (size_t)H * H;
  const float* W3 = b2 + H;
  const float* b3 = W3 + (size_t)H * NO;
  const float* stdv = b3 + NO;

  pol_acc a1[T1], a2[T2], a3[T3];
#pragma unroll
  for (int r = 0; r < 16; r++) {
#pragma unroll
    for (int j = 0; j < T1; j++) a1[j][r] = 0.0f;
#pragma unroll
    for (int j = 0; j < T2; j++) a2[j][r] = 0.0f;
#pragma unroll
    for (int j = 0; j < T3; j++) a3[j][r] = 0.0f;
  }
  // column sums: slot = tid + 256 j of  db1 [H]  db2 [H]  db3 [NO]  dstd [nu]  statistics [8]
  const int n_slots = 2 * H + NO + nu + PGRAD_STATS;
  float csum[2] = {0.0f, 0.0f};
  int coff[2] = {-1, -1}, cpitch[2] = {0, 0};   // the column's first element as an offset into the block's LDS
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int s = tid + PGRAD_THREADS * j;
    if (s >= n_slots) continue;
    if (s < H) { coff[j] = (int)(I1 - lds) + s; cpitch[j] = PH; continue; }
    s -= H;
    if (s < H) { coff[j] = (int)(I2 - lds) + s; cpitch[j] = PH; continue; }
    s -= H;
    cpitch[j] = PD;
    const int base = (int)(DO - lds);
    if (s < NO) { coff[j] = base + s; continue; }
    s -= NO;
    if (s < nu) { coff[j] = base + PGRAD_DO_STD + s; continue; }
    s -= nu;
    coff[j] = base + PGRAD_DO_STAT + s;
  }
  __syncthreads();

  const int64_t n_tiles = (p.total + POLICY_ROWS - 1) / POLICY_ROWS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t g0 = tile * POLICY_ROWS;
    if constexpr (ROWS) {   // (the barrier at the end of the tile before has every reader of SRC behind it)
      if (tid < POLICY_ROWS) {
        int64_t s = -1;
        if (g0 + tid < p.total) {
          const int64_t e = p.rows[g0 + tid];
          if (e >= 0 && e < p.limit) {
            const int64_t plane = e / p.n_rows;
            s = plane * p.pitch + (e - plane * p.n_rows);
          }
        }
        SRC[tid] = s;
      }
      __syncthreads();
    }
    for (int piece = tid; piece < POLICY_ROWS * Q; piece += PGRAD_THREADS) {
      const int r = piece / Q, q = piece - r * Q;
      const int64_t g = g0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // rows at or beyond the last are not read
      if constexpr (ROWS) {
        const int64_t src = SRC[r];
        if (src >= 0) {
          v = *reinterpret_cast<const float4*>(p.obs + (size_t)src * (size_t)p.obs_pitch + 4 * q);
          if constexpr (NORM) v = obs_norm_piece(v, p.table, od, q, p.obs_clip);
        }
      } else if (g < p.total) {
        const int64_t plane = g / p.n_rows;
        const int64_t src = plane * p.pitch + (g - plane * p.n_rows);
        v = *reinterpret_cast<const float4*>(p.obs + (size_t)src * (size_t)p.obs_pitch + 4 * q);
        if constexpr (NORM) v = obs_norm_piece(v, p.table, od, q, p.obs_clip);
      }
      *reinterpret_cast<float4*>(X + r * PX + 4 * q) = v;
    }
    __syncthreads();

    // forward, the chains of k_policy_forward
    for (int m = wave; m < NT; m += PGRAD_WAVES) {
      pol_acc h = pgrad_forward_tile(W1, b1, H, H, od, X, PX, m, col, half);
#pragma unroll
      for (int r = 0; r < 16; r++) h[r] = policy_act(h[r], p.activation);
      pgrad_store_tile(I1, PH, m, h, col, half);
    }
    __syncthreads();
    for (int m = wave; m < NT; m += PGRAD_WAVES) {
      pol_acc h = pgrad_forward_tile(W2, b2, H, H, H, I1, PH, m, col, half);
#pragma unroll
      for (int r = 0; r < 16; r++) h[r] = policy_act(h[r], p.activation);
      pgrad_store_tile(I2, PH, m, h, col, half);
    }
    __syncthreads();
    if (wave == 0) {
      const pol_acc o = pgrad_forward_tile(W3, b3, NO, NO, H, I2, PH, 0, col, half);
      pgrad_store_tile(DO, PD, 0, o, col, half);   // columns 0 ... 31: outputs 0 ... NO - 1, zeros behind them
    }
    __syncthreads();

    // the head gradient, one lane per row
    if (tid < POLICY_ROWS) {
      float* d = DO + tid * PD;
      const int64_t g = g0 + tid;
      const float v = d[nu], cv = d[nu + 1];
      float mean[12];
#pragma unroll
      for (int u = 0; u < 12; u++) mean[u] = u < nu ? d[u] : 0.0f;
#pragma unroll
      for (int k = 0; k < PD; k += 4) *reinterpret_cast<float4*>(d + k) = make_float4(0.f, 0.f, 0.f, 0.f);
      bool present;
      size_t src = 0;
      if constexpr (ROWS) {
        const int64_t s = SRC[tid];
        present = s >= 0;
        src = (size_t)s;
      } else {
        present = g < p.total;
        if (present) {
          const int64_t plane = g / p.n_rows;
          src = (size_t)(plane * p.pitch + (g - plane * p.n_rows));
        }
      }
      if (present) {
        float ss = 0.0f, slog = 0.0f;
        float zeta[12], istd[12];
#pragma unroll
        for (int u = 0; u < 12; u++) {
          zeta[u] = 0.0f; istd[u] = 0.0f;
          if (u < nu) {
            const float sd = stdv[u];
            const float diff = p.actions[src * (size_t)nu + u] - mean[u];
            istd[u] = 1.0f / sd;
            zeta[u] = diff / sd;
            const float sq = zeta[u] * zeta[u];
            ss = ss + sq;
            slog = slog + 0.69314718055994530942f * __builtin_amdgcn_logf(sd);
          }
        }
        const float lc = (float)nu * 0.91893853320467274178f;   // nu / 2 * log(2 pi)
        const float logp = -0.5f * ss - slog - lc;
        const float lpo = p.logp_old[src];
        const float rho = pol_exp2(1.44269504088896340736f * (logp - lpo));
        float A = p.adv_mul * (p.adv[src] - p.adv_sub);
        if (p.cadv) A = A - p.cadv_mul * (p.cadv[src] - p.cadv_sub);
        const float lo = 1.0f - p.clip, hi = 1.0f + p.clip;
        const bool live = (A >= 0.0f && rho <= hi) || (A < 0.0f && rho >= lo);
        const float rc = rho < lo ? lo : (rho > hi ? hi : rho);
        const float surr = (live ? rho : rc) * A;
        const float dlp = live ? -(rho * A) : 0.0f;   // dL / dlogp
#pragma unroll
        for (int u = 0; u < 12; u++)
          if (u < nu) {
            d[u] = dlp * (zeta[u] * istd[u]);
            d[PGRAD_DO_STD + u] = dlp * ((zeta[u] * zeta[u] - 1.0f) * istd[u]) - p.ent * istd[u];
          }
        const float ev = v - p.ret[src];
        d[nu] = p.vf * ev;
        d[PGRAD_DO_STAT + 0] = -surr;
        d[PGRAD_DO_STAT + 1] = 0.5f * (ev * ev);
        if (p.cret) {
          const float ec = cv - p.cret[src];
          d[nu + 1] = p.cvf * ec;
          d[PGRAD_DO_STAT + 2] = 0.5f * (ec * ec);
        }
        d[PGRAD_DO_STAT + 3] = lpo - logp;
        d[PGRAD_DO_STAT + 4] = live ? 0.0f : 1.0f;
        d[PGRAD_DO_STAT + 5] = 1.0f;
      }
    }
    __syncthreads();

    // dW3 = h2^T dO, and dh2 = W3 dO^T kept in registers until every wavefront has read h2
#pragma unroll
    for (int j = 0; j < T3; j++) {
      const int ki = wave + PGRAD_WAVES * j;
      if (ki < NT) a3[j] = pgrad_dw_tile(a3[j], I2, PH, 32 * ki, DO, PD, 0, col, half);
    }
    pol_acc dh[T3];
#pragma unroll
    for (int j = 0; j < T3; j++) {
      const int m = wave + PGRAD_WAVES * j;
#pragma unroll
      for (int r = 0; r < 16; r++) dh[j][r] = 0.0f;
      if (m < NT) {
        const float* w = W3 + (size_t)(32 * m + col) * NO;
#pragma unroll
        for (int s = 0; s < 8; s++) {
          const int k = 2 * s + half;
          dh[j] = pol_mfma(k < NO ? w[k] : 0.0f, DO[col * PD + k], dh[j]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T3; j++) {
      const int m = wave + PGRAD_WAVES * j;
      if (m < NT) pgrad_store_dz(I2, PH, m, dh[j], col, half, p.activation);
    }
    __syncthreads();

    // dh1 = W2 dz2^T (registers), dW2 = h1^T dz2
#pragma unroll
    for (int j = 0; j < T3; j++) {
      const int m = wave + PGRAD_WAVES * j;
#pragma unroll
      for (int r = 0; r < 16; r++) dh[j][r] = 0.0f;
      if (m < NT) {
        const float* w = W2 + (size_t)(32 * m + col) * H + 4 * half;
        const float* z = I2 + col * PH + 4 * half;
#pragma unroll 4
        for (int q = 0; q < H / 8; q++) {
          const float4 b = *reinterpret_cast<const float4*>(z + 8 * q);
          const float w0 = w[8 * q], w1 = w[8 * q + 1], w2 = w[8 * q + 2], w3 = w[8 * q + 3];
          dh[j] = pol_mfma(w0, b.x, dh[j]);
          dh[j] = pol_mfma(w1, b.y, dh[j]);
          dh[j] = pol_mfma(w2, b.z, dh[j]);
          dh[j] = pol_mfma(w3, b.w, dh[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < T2; j++) {
      const int t = wave + PGRAD_WAVES * j;
      if (t < NT * NT) a2[j] = pgrad_dw_tile(a2[j], I1, PH, 32 * (t / NT), I2, PH, 32 * (t % NT), col, half);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T3; j++) {
      const int m = wave + PGRAD_WAVES * j;
      if (m < NT) pgrad_store_dz(I1, PH, m, dh[j], col, half, p.activation);
    }
    __syncthreads();

    // dW1 = x^T dz1 and the column sums
#pragma unroll
    for (int j = 0; j < T1; j++) {
      const int t = wave + PGRAD_WAVES * j;
      if (t < KT1 * NT) a1[j] = pgrad_dw_tile(a1[j], X, PX, 32 * (t / NT), I1, PH, 32 * (t % NT), col, half);
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (coff[j] >= 0) {
#pragma unroll 8
        for (int row = 0; row < POLICY_ROWS; row++) csum[j] = csum[j] + lds[coff[j] + row * cpitch[j]];
      }
    __syncthreads();   // the next tile overwrites the images
  }

  // the block's partial, every word written by exactly one lane
  float* part = p.part + (size_t)blockIdx.x * (size_t)(p.n_params + PGRAD_STATS);
  float* gb1 = part + (size_t)od * H;
  float* gW2 = gb1 + H;
  float* gb2 = gW2 + (size_t)H * H;
  float* gW3 = gb2 + H;
  float* gb3 = gW3 + (size_t)H * NO;
#pragma unroll
  for (int j = 0; j < T1; j++) {
    const int t = wave + PGRAD_WAVES * j;
    if (t < KT1 * NT) pgrad_put_tile(part, H, od, H, t / NT, t % NT, a1[j], col, half);
  }
#pragma unroll
  for (int j = 0; j < T2; j++) {
    const int t = wave + PGRAD_WAVES * j;
    if (t < NT * NT) pgrad_put_tile(gW2, H, H, H, t / NT, t % NT, a2[j], col, half);
  }
#pragma unroll
  for (int j = 0; j < T3; j++) {
    const int ki = wave + PGRAD_WAVES * j;
    if (ki < NT) pgrad_put_tile(gW3, NO, H, NO, ki, 0, a3[j], col, half);
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int s = tid + PGRAD_THREADS * j;
    if (s >= n_slots) continue;
    if (s < H) { gb1[s] = csum[j]; continue; }
    s -= H;
    if (s < H) { gb2[s] = csum[j]; continue; }
    s -= H;
    gb3[s] = csum[j];   // b3, std and the statistics are contiguous behind W3
  }
}

// d_grad[i] = (accumulate ? d_grad[i] : 0) + scale * part[0][i] + scale * part[1][i] + ... in ascending block order
__global__ __launch_bounds__(256) void k_policy_grad_reduce(const float* part, int n_blocks, int n_words, float scale, int accumulate, float* grad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_words) return;
  float s = accumulate ? grad[i] : 0.0f;
  for (int b = 0; b < n_blocks; b++) {
    const float t = scale * part[(size_t)b * n_words + i];
    s = s + t;
  }
  grad[i] = s;
}

struct AdamArgs {
  int32_t n, clamp_first;
  float beta1, beta2, omb1, omb2, eps, step, clamp_lo;
  float* param; const float* grad; float* m; float* v;
};

__global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const float g = a.grad[i];
  const float m0 = a.beta1 * a.m[i], m1 = a.omb1 * g;
  const float m = m0 + m1;
  const float v0 = a.beta2 * a.v[i], v1 = a.omb2 * g, v2 = v1 * g;
  const float v = v0 + v2;
  const float den = sqrtf(v) + a.eps;
  const float num = a.step * m;
  const float q = num / den;
  float pn = a.param[i] - q;
  if (i >= a.clamp_first) pn = pn > a.clamp_lo ? pn : a.clamp_lo;   // (a NaN parameter becomes clamp_lo)
  a.m[i] = m; a.v[i] = v; a.param[i] = pn;
}

}  // namespace sag

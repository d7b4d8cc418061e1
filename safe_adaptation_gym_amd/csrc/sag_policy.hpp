// sag_policy.hpp - the learner's half of a model-free rollout on the context stream: one fused forward of a Gaussian
// actor-critic MLP (sag_policy_forward_device; include/sag.h defines the arithmetic).
//   k_policy_forward<NT>   obs [n_rows][obs_dim] -> hidden -> hidden -> nu + 2 outputs (action mean, value, cost value),
//                          hidden = 32 * NT; sampling and log-probability in the same launch; no activation leaves the CU
//   k_policy_forward<NT, true>   the same with every observation element normalised and clamped where its row is staged
//                          (sag_policy_forward_norm_device; sag_obs_norm.hpp has the arithmetic)
// One wavefront per 32 rows.  Every product runs on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: D = A[32][2] * B[2][32] + C,
// bit for bit fma(a1, b1, fma(a0, b0, c)), one rounding per product), in the orientation D^T = W^T * X^T: the weights are the
// A operand (lane l: unit row l & 31, k = l >> 5), the activations the B operand (lane l: row l & 31, k = l >> 5).  A result
// tile then has the row (the env) on the lane and 16 of the 32 unit rows in the 16 accumulator registers - register r of lane
// half h is tile row (r & 3) + 8 * (r >> 2) + 4 * h - and IS the B operand of the next layer with no lane movement and no LDS:
// register r is k-step r, half h its k.  Summed that way the tile rows are visited in the order 0, 4, 1, 5, 2, 6, 3, 7, 8, 12 ...;
// the header's chain is in ascending k, so tile row rho of tile m holds hidden unit 32 m + tile_unit(rho), the inverse of that
// order.  The placement is an address computation on the weight loads (hidden-unit labels are free inside the kernel) and
// parameters stay in natural layout: lane (row, half) holds unit 32 m + 2 r + half in register r of tile m, which is exactly
// the k that k-step 16 m + r of the next layer asks of it.  The head keeps natural labels (tile row = output index).
// The observations are staged once in LDS with coalesced 16-byte pieces (the walk of k_save_rows) because lane (row, half)
// needs the even or the odd elements of its own row; weights are read from global memory (L2) as one dword per lane and MFMA.
#pragma once
#include "sag_device.hpp"
#include "sag_obs_norm.hpp"

namespace sag {

// Counter word 3 of the policy's draws: stream 5, above the 26 bits of streams 0 - 3 as the planner's stream 4 is.
constexpr uint32_t POLICY_STREAM_WORD = 5u << 26;
constexpr int POLICY_ROWS = 32;                 // rows per wavefront: the MFMA's 32 columns
constexpr int POLICY_MAX_TILES = 8;             // hidden <= 256
constexpr int POLICY_MAX_OBS = 104;
// The staged tile is 32 rows x obs_dim floats at a row pitch of 4 (mod 8) floats: the 64 lanes' reads of one k-step (lane
// (row, half) reads element 2 ks + half of its row) meet two to a bank, and rows stay 16-byte aligned for the staging stores.
inline int policy_lds_pitch(int obs_dim) { return obs_dim + ((obs_dim & 7) ? 0 : 4); }

#if SAG_HOSTEMU
// The host build has no ext_vector_type and no MFMA builtin: the accumulator is a plain struct and the instruction is its
// definition over the wavefront's fibers.  Everything else below - lane maps, unit placement, addresses - is the device's.
struct pol_acc {
  float v[16];
  float& operator[](int i) { return v[i]; }
  const float& operator[](int i) const { return v[i]; }
};
static inline pol_acc pol_mfma(float a, float b, pol_acc c) {
  const int lane = (int)threadIdx.x & 63;
  const float b0 = __shfl(b, lane & 31), b1 = __shfl(b, (lane & 31) + 32);
  for (int r = 0; r < 16; r++) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const float a0 = __shfl(a, row), a1 = __shfl(a, row + 32);
    c[r] = fmaf(a0, b0, c[r]);
    c[r] = fmaf(a1, b1, c[r]);
  }
  return c;
}
static inline float pol_exp2(float x) { return exp2f(x); }
#else
typedef float pol_acc __attribute__((ext_vector_type(16)));
__device__ __forceinline__ pol_acc pol_mfma(float a, float b, pol_acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float pol_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
#endif

struct PolicyArgs {
  int32_t n_rows, obs_dim, nu, activation, mean_only, obs_pitch, lds_pitch;
  uint32_t id0, draw, k0, k1;   // counter word 0 of row 0, word 1, the context key
  float logp_const;
  const float* params;
  const float* obs;
  float* actions; float* logp; float* value; float* cvalue;
};
// sag_policy_forward_norm_device: the same, with every staged observation element normalised under `table`
struct PolicyNormArgs : PolicyArgs {
  const float* table;   // mean [obs_dim], rstd [obs_dim]
  float obs_clip;
};

// the hidden unit (0 ... 31, inside its block of 32) that sits in tile row rho: the position of rho in 0, 4, 1, 5, ...
__device__ inline int policy_tile_unit(int rho) { return 2 * ((rho & 3) + 4 * (rho >> 3)) + ((rho >> 2) & 1); }

// relu: x > 0 ? x : 0.  tanh: 1 - 2 / (exp2(2 log2(e) x) + 1) with the hardware exp2 and reciprocal, each operation rounded
// on its own (include/sag.h states the form).
__device__ inline float policy_act(float x, int activation) {
  if (activation == 0) return x > 0.0f ? x : 0.0f;
  const float e = pol_exp2(2.88539008177792681472f * x);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

template <bool NORM> struct PolicyArgsOf { typedef PolicyArgs type; };
template <> struct PolicyArgsOf<true> { typedef PolicyNormArgs type; };

// NORM: sag_policy_forward_norm_device; the plain instances are what they were before the switch existed
template <int NT, bool NORM = false>
__global__ __launch_bounds__(WAVE) void k_policy_forward(typename PolicyArgsOf<NORM>::type p) {
#pragma clang fp contract(off)
  constexpr int H = 32 * NT;
  HIP_DYNAMIC_SHARED(float4, tile4)   // POLICY_ROWS * lds_pitch floats: sized for the robot, so that LDS does not bound the occupancy
  float* tile = reinterpret_cast<float*>(tile4);
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const size_t row0 = (size_t)blockIdx.x * POLICY_ROWS;
  const int od = p.obs_dim, nu = p.nu, NO = nu + 2;
  const int Q = od >> 2, LP = p.lds_pitch;
  for (int piece = lane; piece < POLICY_ROWS * Q; piece += WAVE) {
    const int r = piece / Q, q = piece - r * Q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // rows at or beyond n_rows are not read
    if (row0 + (size_t)r < (size_t)p.n_rows) {
      v = *reinterpret_cast<const float4*>(p.obs + (row0 + (size_t)r) * (size_t)p.obs_pitch + 4 * q);
      if constexpr (NORM) v = obs_norm_piece(v, p.table, od, q, p.obs_clip);
    }
    *reinterpret_cast<float4*>(tile + r * LP + 4 * q) = v;
  }
  __syncthreads();

  const float* W1 = p.params;
  const float* b1 = W1 + (size_t)od * H;
  const float* W2 = b1 + H;
  const float* b2 = W2 + (size_t)H * H;
  const float* W3 = b2 + H;
  const float* b3 = W3 + (size_t)H * NO;
  const float* stdv = b3 + NO;
  const int pu = policy_tile_unit(col);   // as the A operand, lane l feeds tile row l & 31: its unit inside a block of 32

  // Weight loads run D k-steps ahead of the MFMAs that use them, in a register ring: a step's NT MFMAs are 64 NT cycles of
  // cover, a load from L2 takes some 800, and with few wavefronts per SIMD nothing else hides it.  D * NT ~ 16 dwords in flight.
  constexpr int D = 16 / NT < 2 ? 2 : 16 / NT;

  // layer 1: k-step s is k = 2 s + half, the activations come from LDS
  pol_acc h1[NT];
#pragma unroll
  for (int m = 0; m < NT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) h1[m][r] = b1[32 * m + 2 * r + half];
  {
    const int S = od >> 1;   // 30, 36 or 52: more than D
    float wr[D][NT], br[D];
#pragma unroll
    for (int j = 0; j < D; j++) {
      const int k = 2 * j + half;
      br[j] = tile[col * LP + k];
#pragma unroll
      for (int m = 0; m < NT; m++) wr[j][m] = W1[(size_t)k * H + pu + 32 * m];
    }
    for (int s0 = 0; s0 < S; s0 += D) {
#pragma unroll
      for (int j = 0; j < D; j++) {
        if (s0 + j < S) {   // (wave-uniform; false in the last pass only)
          float wc[NT];
#pragma unroll
          for (int m = 0; m < NT; m++) wc[m] = wr[j][m];
          const float bc = br[j];
          const int k = 2 * min(s0 + j + D, S - 1) + half;   // past the end: the last step again, never used
          br[j] = tile[col * LP + k];
#pragma unroll
          for (int m = 0; m < NT; m++) wr[j][m] = W1[(size_t)k * H + pu + 32 * m];
#pragma unroll
          for (int m = 0; m < NT; m++) h1[m] = pol_mfma(wc[m], bc, h1[m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < NT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) h1[m][r] = policy_act(h1[m][r], p.activation);

  // layer 2: register r of tile mk is k-step s = 16 mk + r
  pol_acc h2[NT];
#pragma unroll
  for (int m = 0; m < NT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) h2[m][r] = b2[32 * m + 2 * r + half];
  {
    constexpr int S = 16 * NT;
    float wr[D][NT];
#pragma unroll
    for (int j = 0; j < D; j++)
#pragma unroll
      for (int m = 0; m < NT; m++) wr[j][m] = W2[(size_t)(2 * j + half) * H + pu + 32 * m];
#pragma unroll
    for (int s = 0; s < S; s++) {
      float wc[NT];
#pragma unroll
      for (int m = 0; m < NT; m++) wc[m] = wr[s % D][m];
      if (s + D < S) {
#pragma unroll
        for (int m = 0; m < NT; m++) wr[s % D][m] = W2[(size_t)(2 * (s + D) + half) * H + pu + 32 * m];
      }
      const float b = h1[s >> 4][s & 15];
#pragma unroll
      for (int m = 0; m < NT; m++) h2[m] = pol_mfma(wc[m], b, h2[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < NT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) h2[m][r] = policy_act(h2[m][r], p.activation);

  // head: tile row = output index, rows at or beyond nu + 2 carry zeros; one dependent MFMA per k-step, 16 loads ahead
  pol_acc o;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int rho = (r & 3) + 8 * (r >> 2) + 4 * half;
    o[r] = rho < NO ? b3[rho] : 0.0f;
  }
  {
    constexpr int S = 16 * NT;
    float ar[16];
#pragma unroll
    for (int j = 0; j < 16; j++) ar[j] = col < NO ? W3[(size_t)(2 * j + half) * NO + col] : 0.0f;
#pragma unroll
    for (int s = 0; s < S; s++) {
      const float a = ar[s & 15];
      if (s + 16 < S) ar[s & 15] = col < NO ? W3[(size_t)(2 * (s + 16) + half) * NO + col] : 0.0f;
      o = pol_mfma(a, h2[s >> 4][s & 15], o);
    }
  }

  const size_t row = row0 + (size_t)col;
  if (row >= (size_t)p.n_rows) return;

  // The normals: element u of the row is element u % 4 of Philox block u / 4.  Registers 4 g ... 4 g + 3 of this lane hold outputs
  // 8 g + 4 half ... + 3, the elements of block 2 g + half; the sum of squares runs over every block, in ascending u.
  float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ss = 0.0f;
  const bool sample = p.actions != nullptr && !p.mean_only;
  if (sample) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      if (4 * q < nu) {
        uint32_t c[4] = {p.id0 + (uint32_t)row, p.draw, (uint32_t)q, POLICY_STREAM_WORD};
        philox4x32_10(c, p.k0, p.k1);
        float zq[4];
        box_muller(c[0], c[1], zq[0], zq[1]);
        box_muller(c[2], c[3], zq[2], zq[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (4 * q + j < nu) { const float sq = zq[j] * zq[j]; ss = ss + sq; }
          if (q == half) z[j] = zq[j];
          if (q == 2 + half) z[4 + j] = zq[j];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {   // outputs 0 ... 15: registers 8 ... 15 are rows 16 ... 31
    const int rho = (r & 3) + 8 * (r >> 2) + 4 * half;
    const float v = o[r];
    if (rho < nu) {
      if (p.actions) { const float sz = stdv[rho] * z[r]; p.actions[row * (size_t)nu + rho] = v + sz; }   // unclamped
    } else if (rho == nu) {
      if (p.value) p.value[row] = v;
    } else if (rho == nu + 1) {
      if (p.cvalue) p.cvalue[row] = v;
    }
  }
  if (half == 0 && p.logp) { const float hs = 0.5f * ss; p.logp[row] = -hs - p.logp_const; }
}

}  // namespace sag

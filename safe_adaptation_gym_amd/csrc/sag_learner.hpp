// sag_learner.hpp - what the learner needs around the backward pass, on the context stream (include/sag.h defines the four
// functions): deterministic fp32 reductions over pitched device arrays whose results stay on the device.
//   k_learn_partial<MODE>   one partial (sum, count) per block over chunks of LEARN_UNIT logical elements
//                           MODE 0: sum of x   1: sum of (x - mean)^2, mean read from out[1]   2: sum of x^2
//   k_moments_final         the partials added in ascending block order -> count, mean (pass 0) or var, rstd (pass 1)
//   k_advantage_mix         out = norm(adv) - lambda * norm(cadv), elementwise, every operation rounded on its own
//   k_lagrange              the multiplier's projected ascent step, one thread
//   k_grad_clip_scale       every block re-adds the partials of MODE 2 in ascending order, then scales its share
// Logical element e (0 <= e < n_planes * n_rows) is row e % n_rows of plane e / n_rows; its float offset is
// (plane * pitch + row) * stride.  A chunk is LEARN_UNIT consecutive logical elements: LEARN_QUADS rounds in which thread t
// takes the four elements 4 (256 j + t) ... + 3 of the chunk, as one 16-byte load where stride is 1, the four lie in one
// plane and the address is 16-byte aligned, and as four dword loads otherwise.  Pad rows, the other columns of a strided
// row and elements under a zero mask byte are never loaded into a register that the arithmetic reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sag {

constexpr int LEARN_THREADS = 256;
constexpr int LEARN_QUADS = 4;                                    // 16-byte loads in flight per thread
constexpr int LEARN_UNIT = LEARN_THREADS * 4 * LEARN_QUADS;       // 4096 elements: a block's unit of work
constexpr int LEARN_DEFAULT_BLOCKS = 256;                         // one per CU of an MI355X
constexpr int LEARN_MAX_BLOCKS = 1024;

// the grid: a function of the number of elements and max_blocks only
inline int learn_grid(int64_t total, int max_blocks) {
  const int64_t chunks = (total + LEARN_UNIT - 1) / LEARN_UNIT;
  const int64_t cap = max_blocks > 0 ? (max_blocks < LEARN_MAX_BLOCKS ? max_blocks : LEARN_MAX_BLOCKS) : LEARN_DEFAULT_BLOCKS;
  return (int)(chunks < cap ? chunks : cap);
}

struct LearnSpan {
  uint32_t total, n_rows, pitch, stride;   // total = n_planes * n_rows < 2^31
};

// float offset (before the stride) of logical element e, and how many elements from e on lie in the same plane
__device__ inline size_t learn_offset(const LearnSpan& s, uint32_t e, uint32_t& run) {
  if (s.pitch == s.n_rows) { run = s.total - e; return e; }
  const uint32_t p = e / s.n_rows, r = e - p * s.n_rows;
  run = s.n_rows - r;
  return (size_t)p * s.pitch + r;
}

struct LearnPartialArgs {
  LearnSpan span;
  uint32_t x_mis, m_mis;     // (address of x / 4) & 3, (address of mask) & 3: which offsets are 16- / 4-byte aligned
  const float* x; const uint8_t* mask;
  const float* mom;          // MODE 1: the moments array whose word 1 is the mean
  float* part_sum; int32_t* part_cnt;   // [gridDim.x] each
};

template <int MODE>
__device__ inline float learn_term(float x, float mean) {
#pragma clang fp contract(off)
  if (MODE == 0) return x;
  if (MODE == 1) { const float d = x - mean; return d * d; }
  return x * x;
}

template <int MODE>
__global__ __launch_bounds__(LEARN_THREADS) void k_learn_partial(LearnPartialArgs a) {
#pragma clang fp contract(off)
  __shared__ float wsum[LEARN_THREADS / 64];
  __shared__ int wcnt[LEARN_THREADS / 64];
  const int tid = threadIdx.x;
  const LearnSpan s = a.span;
  const float mean = MODE == 1 ? a.mom[1] : 0.0f;
  const uint32_t chunks = (s.total + LEARN_UNIT - 1) / LEARN_UNIT;
  float sum = 0.0f;
  int cnt = 0;
  for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    float v[LEARN_QUADS][4];
    int take[LEARN_QUADS];   // bit k: element k of the quad counts
#pragma unroll
    for (int j = 0; j < LEARN_QUADS; j++) {
      const uint32_t e = c * (uint32_t)LEARN_UNIT + 4u * (uint32_t)(j * LEARN_THREADS + tid);
      take[j] = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) v[j][k] = 0.0f;
      if (e >= s.total) continue;
      uint32_t run;
      const size_t off = learn_offset(s, e, run);
      if (run >= 4) {   // four elements of one plane
        int m = 15;
        if (a.mask) {
          if (((off + a.m_mis) & 3) == 0) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(a.mask + off);
            m = ((w & 0xffu) ? 1 : 0) | ((w & 0xff00u) ? 2 : 0) | ((w & 0xff0000u) ? 4 : 0) | ((w & 0xff000000u) ? 8 : 0);
          } else {
            m = (a.mask[off] ? 1 : 0) | (a.mask[off + 1] ? 2 : 0) | (a.mask[off + 2] ? 4 : 0) | (a.mask[off + 3] ? 8 : 0);
          }
        }
        take[j] = m;
        if (m == 0) continue;
        if (s.stride == 1 && ((off + a.x_mis) & 3) == 0) {
          const float4 q = *reinterpret_cast<const float4*>(a.x + off);
          v[j][0] = (m & 1) ? q.x : 0.0f; v[j][1] = (m & 2) ? q.y : 0.0f; v[j][2] = (m & 4) ? q.z : 0.0f; v[j][3] = (m & 8) ? q.w : 0.0f;
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++)
            if (m & (1 << k)) v[j][k] = a.x[(off + k) * s.stride];
        }
      } else {          // the quad crosses a plane's end (or the array's): element by element
        for (uint32_t k = 0; k < 4 && e + k < s.total; k++) {
          uint32_t r1;
          const size_t o = learn_offset(s, e + k, r1);
          if (a.mask && !a.mask[o]) continue;
          take[j] |= 1 << k;
          v[j][k] = a.x[o * s.stride];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < LEARN_QUADS; j++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (take[j] & (1 << k)) { sum = sum + learn_term<MODE>(v[j][k], mean); cnt += 1; }
  }
  // lanes, then the four wavefronts in ascending order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float os = __shfl_xor(sum, d);
    const int oc = __shfl_xor(cnt, d);
    sum = sum + os; cnt += oc;
  }
  if ((tid & 63) == 0) { wsum[tid >> 6] = sum; wcnt[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    float t = wsum[0];
    int n = wcnt[0];
    for (int w = 1; w < LEARN_THREADS / 64; w++) { t = t + wsum[w]; n += wcnt[w]; }
    a.part_sum[blockIdx.x] = t;
    a.part_cnt[blockIdx.x] = n;
  }
}

// the block's partials staged in LDS by all threads, then added by thread 0 in ascending block order
__device__ inline void learn_add_partials(const float* part_sum, const int32_t* part_cnt, int n_blocks, float* lds_sum, int* lds_cnt,
                                          float& sum, int& cnt) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < n_blocks; b += blockDim.x) {
    lds_sum[b] = part_sum[b];
    if (part_cnt) lds_cnt[b] = part_cnt[b];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
    int n = 0;
    for (int b = 0; b < n_blocks; b++) {
      t = t + lds_sum[b];
      if (part_cnt) n += lds_cnt[b];
    }
    lds_sum[0] = t;
    if (part_cnt) lds_cnt[0] = n;
  }
  __syncthreads();
  sum = lds_sum[0];
  cnt = part_cnt ? lds_cnt[0] : 0;
}

// pass 0: out = {count, sum / count, 0, 0};  pass 1: out[2] = sum / count, out[3] = 1 / (sqrt(out[2]) + eps); count == 0: zeros
__global__ __launch_bounds__(LEARN_THREADS) void k_moments_final(const float* part_sum, const int32_t* part_cnt, int n_blocks, int pass,
                                                                 float eps, float* out) {
#pragma clang fp contract(off)
  __shared__ float lds_sum[LEARN_MAX_BLOCKS];
  __shared__ int lds_cnt[LEARN_MAX_BLOCKS];
  float sum;
  int cnt;
  learn_add_partials(part_sum, pass == 0 ? part_cnt : nullptr, n_blocks, lds_sum, lds_cnt, sum, cnt);
  if (threadIdx.x != 0) return;
  if (pass == 0) {
    const float n = (float)cnt;
    out[0] = n;
    out[1] = cnt > 0 ? sum / n : 0.0f;
    out[2] = 0.0f; out[3] = 0.0f;
  } else {
    const float n = out[0];
    if (n > 0.0f) {
      const float var = sum / n;
      const float den = sqrtf(var) + eps;
      out[2] = var;
      out[3] = 1.0f / den;
    }
  }
}

struct MixArgs {
  LearnSpan span;
  uint32_t mis;              // 0 where adv, cadv and out are all 16-byte aligned
  int32_t adv_mode, cadv_mode;
  float cost_weight;
  const float* adv; const float* cadv; const float* adv_mom; const float* cadv_mom; const float* lambda;
  float* out;
};

__device__ inline float mix_norm(float x, int mode, float m, float s) {
#pragma clang fp contract(off)
  if (mode >= 1) x = x - m;
  if (mode == 2) x = x * s;
  return x;
}

__global__ __launch_bounds__(LEARN_THREADS) void k_advantage_mix(MixArgs a) {
#pragma clang fp contract(off)
  const LearnSpan s = a.span;
  const uint64_t q = (uint64_t)blockIdx.x * LEARN_THREADS + threadIdx.x;
  if (4 * q >= s.total) return;
  const uint32_t e = (uint32_t)(4 * q);
  const float ma = a.adv_mode ? a.adv_mom[1] : 0.0f, sa = a.adv_mode ? a.adv_mom[3] : 1.0f;
  const bool cost = a.cadv != nullptr;
  const float mc = cost && a.cadv_mode ? a.cadv_mom[1] : 0.0f, sc = cost && a.cadv_mode ? a.cadv_mom[3] : 1.0f;
  const float lam = a.lambda ? a.lambda[0] : a.cost_weight;
  uint32_t run;
  const size_t off = learn_offset(s, e, run);
  if (run >= 4 && a.mis == 0 && (off & 3) == 0) {
    const float4 x = *reinterpret_cast<const float4*>(a.adv + off);
    float4 r;
    r.x = mix_norm(x.x, a.adv_mode, ma, sa); r.y = mix_norm(x.y, a.adv_mode, ma, sa);
    r.z = mix_norm(x.z, a.adv_mode, ma, sa); r.w = mix_norm(x.w, a.adv_mode, ma, sa);
    if (cost) {
      const float4 c = *reinterpret_cast<const float4*>(a.cadv + off);
      const float t0 = lam * mix_norm(c.x, a.cadv_mode, mc, sc), t1 = lam * mix_norm(c.y, a.cadv_mode, mc, sc);
      const float t2 = lam * mix_norm(c.z, a.cadv_mode, mc, sc), t3 = lam * mix_norm(c.w, a.cadv_mode, mc, sc);
      r.x = r.x - t0; r.y = r.y - t1; r.z = r.z - t2; r.w = r.w - t3;
    }
    *reinterpret_cast<float4*>(a.out + off) = r;
    return;
  }
  for (uint32_t k = 0; k < 4 && e + k < s.total; k++) {
    uint32_t r1;
    const size_t o = learn_offset(s, e + k, r1);
    float r = mix_norm(a.adv[o], a.adv_mode, ma, sa);
    if (cost) {
      const float t = lam * mix_norm(a.cadv[o], a.cadv_mode, mc, sc);
      r = r - t;
    }
    a.out[o] = r;
  }
}

// state = {lambda, last mean cost, last episode count, updates taken}
__global__ void k_lagrange(const float* mom, float lr, float budget, float lambda_max, float* state) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float n = mom[0];
  if (n > 0.0f) {
    const float mean = mom[1];
    const float d = mean - budget;
    const float step = lr * d;
    float l = state[0] + step;
    l = l > 0.0f ? l : 0.0f;               // (a NaN becomes 0)
    l = l < lambda_max ? l : lambda_max;
    state[0] = l; state[1] = mean; state[2] = n; state[3] = state[3] + 1.0f;
  } else {
    state[2] = 0.0f;
  }
}

// norm = sqrt(sum of the partials in ascending block order), factor = min(1, max_norm / (norm + 1e-6)); g *= factor
__global__ __launch_bounds__(LEARN_THREADS) void k_grad_clip_scale(const float* part_sum, int n_blocks, float max_norm, uint32_t n, float* grad,
                                                                   float* out) {
#pragma clang fp contract(off)
  __shared__ float lds_sum[LEARN_MAX_BLOCKS];
  float sum;
  int cnt;
  learn_add_partials(part_sum, nullptr, n_blocks, lds_sum, nullptr, sum, cnt);
  const float norm = sqrtf(sum);
  const float den = norm + 1e-6f;
  const float f = max_norm / den;
  const float factor = f > 1.0f ? 1.0f : f;   // (a NaN stays: it reaches every element, as the convention's clamp does)
  if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = norm; out[1] = factor; }
  if (factor == 1.0f) return;
  const uint32_t chunks = (n + LEARN_UNIT - 1) / LEARN_UNIT;
  for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x)
    for (int j = 0; j < 4 * LEARN_QUADS; j++) {
      const uint32_t e = c * (uint32_t)LEARN_UNIT + (uint32_t)(j * LEARN_THREADS) + threadIdx.x;
      if (e < n) grad[e] = grad[e] * factor;
    }
}

}  // namespace sag

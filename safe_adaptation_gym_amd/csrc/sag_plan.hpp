// sag_plan.hpp - the device half of a shooting planner over the simulator itself (constrained CEM): with sag_fork_device
// (every real env broadcast to K candidates) and the step, a whole planning iteration stays on the context stream.
//   k_plan_sample      K candidate action sequences per group from mean / sigma (sag_plan_sample_device)
//   k_plan_accumulate  discounted return, cost, steps alive and goals met of a scoring rollout, after each of its steps
//   k_plan_refit       rank the K candidates of a group under its cost budget, refit mean / sigma to the E elites
//   k_plan_shift       receding-horizon warm start          k_plan_clear   mean = 0, sigma = sigma_init for chosen groups
// Layouts (fp32, h-major: step t's actions are one contiguous [N][nu] block - what the step reads - and the first action of
// the mean is contiguous): plans [H][N][nu], mean / sigma [H][G][nu], score [N] float4.  Groups are consecutive: candidate k
// of group g is env g * K + k, G = N / K.
#pragma once
#include "sag_device.hpp"

namespace sag {

// Counter word 3 of the planner's draws: stream 4, in the bits above the 26 (episode nonce << 2 | stream) that streams 0 - 3
// use, so that no (nonce, stream) word of theirs equals it.
constexpr uint32_t PLAN_STREAM_WORD = 4u << 26;
constexpr int PLAN_REFIT_THREADS = 256;

// One lane per (env, block of four consecutive (h, u) elements; element e = h * nu + u): Philox block
// (id0 + i, draw, e / 4, PLAN_STREAM_WORD) under the context key, elements 4q, 4q + 1 = the two normals of box_muller(words
// 0, 1), elements 4q + 2, 4q + 3 those of box_muller(words 2, 3).  Candidate 0 of a group is the mean itself (z = 0).
// The env index runs fastest: a wavefront writes neighbouring envs of one step.
__global__ __launch_bounds__(256) void k_plan_sample(int N, int K, int H, int nu, uint32_t id0, uint32_t draw, uint32_t k0, uint32_t k1,
                                                      const float* __restrict__ mean, const float* __restrict__ sigma,
                                                      float* __restrict__ plans) {
  const int E = H * nu, Q = (E + 3) >> 2;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)Q * (size_t)N) return;
  const int q = (int)(t / (size_t)N), i = (int)(t % (size_t)N);
  const int g = i / K, G = N / K;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (i - g * K != 0) {
    uint32_t c[4] = {id0 + (uint32_t)i, draw, (uint32_t)q, PLAN_STREAM_WORD};
    philox4x32_10(c, k0, k1);
    box_muller(c[0], c[1], z[0], z[1]);
    box_muller(c[2], c[3], z[2], z[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = 4 * q + j;
    if (e < E) {
      const int h = e / nu, u = e - h * nu;
      const size_t m = ((size_t)h * G + g) * nu + u;
      const float v = mean[m] + sigma[m] * z[j];
      plans[((size_t)h * N + i) * nu + u] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
}

// One lane per env, after a step of a scoring rollout: 8 + 3 B, one byte and one float4 in, the float4 and the byte out.
// score = {discounted return, discounted cost, steps alive, goals met}.  An env is alive until a step reports done; that
// step is counted (as k_episode_track counts the final transition).  The multiply and the add stay two fp32 operations:
// NumPy restates them bit for bit.
__global__ __launch_bounds__(256) void k_plan_accumulate(int N, float w, const float* __restrict__ reward, const uint8_t* __restrict__ cost,
                                                          const uint8_t* __restrict__ done, const uint8_t* __restrict__ met,
                                                          uint8_t* __restrict__ alive, float4* __restrict__ score) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (!alive[i]) return;
  float4 s = score[i];
  const float wr = w * reward[2 * (size_t)i];
  const float wc = w * (cost[i] != 0 ? 1.0f : 0.0f);
  s.x = s.x + wr;
  s.y = s.y + wc;
  s.z += 1.0f;
  s.w += met[i] != 0 ? 1.0f : 0.0f;
  score[i] = s;
  if (done[i]) alive[i] = 0;
}

__device__ inline bool plan_finite(float x) { return (__float_as_int(x) & 0x7f800000) != 0x7f800000; }

// the class of a candidate: 0 feasible, 1 infeasible, 2 a non-finite return or cost
__device__ inline int plan_class(float ret, float cost, bool has_budget, float budget) {
  if (!plan_finite(ret) || !plan_finite(cost)) return 2;
  return !has_budget || cost <= budget ? 0 : 1;
}

// the total order: does candidate a come before candidate b?
__device__ inline bool plan_before(int ca, float ra, float qa, int ka, int cb, float rb, float qb, int kb) {
  if (ca != cb) return ca < cb;
  if (ca == 0) return ra > rb || (ra == rb && ka < kb);
  if (ca == 1) return qa < qb || (qa == qb && (ra > rb || (ra == rb && ka < kb)));
  return ka < kb;
}

// One workgroup per group.  Rank of a candidate = how many candidates come before it in the total order (feasible first,
// among them the higher return; among infeasible ones the lower cost, then the higher return; ties: the lower k; non-finite
// last, by k): a permutation of 0 .. K - 1, computed with the (return, cost) pairs staged in LDS a tile of 256 at a time -
// K * K comparisons, K in the hundreds.  Every loop bound is uniform over the workgroup, so K may exceed it.  The ranks go to
// `rank` (context-owned, [N]); then one lane per (h, u) element sums the elites' values in ascending k - one fp32 chain per
// element, so the result does not depend on the launch shape - and a second pass takes the mean squared deviation.
__global__ __launch_bounds__(PLAN_REFIT_THREADS) void k_plan_refit(int N, int K, int H, int nu, int E, const float* __restrict__ plans,
                                                                    const float4* __restrict__ score, const float* __restrict__ budget,
                                                                    float sigma_min, int32_t* __restrict__ rank, float* __restrict__ mean,
                                                                    float* __restrict__ sigma, int32_t* __restrict__ best,
                                                                    float4* __restrict__ best_score) {
  __shared__ float t_ret[PLAN_REFIT_THREADS], t_cost[PLAN_REFIT_THREADS];
  __shared__ int t_cls[PLAN_REFIT_THREADS];
  const int g = blockIdx.x, G = N / K, tid = threadIdx.x;
  const size_t base = (size_t)g * K;
  const bool has_budget = budget != nullptr;
  const float bud = has_budget ? budget[g] : 0.0f;
  for (int k0 = 0; k0 < K; k0 += PLAN_REFIT_THREADS) {
    const int k = k0 + tid;
    const bool mine = k < K;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mine) s = score[base + k];
    const int cls = plan_class(s.x, s.y, has_budget, bud);
    int r = 0;
    for (int j0 = 0; j0 < K; j0 += PLAN_REFIT_THREADS) {
      __syncthreads();   // (the tile of the pass before has been read)
      if (j0 + tid < K) {
        const float4 o = j0 == k0 ? s : score[base + j0 + tid];
        t_ret[tid] = o.x; t_cost[tid] = o.y; t_cls[tid] = plan_class(o.x, o.y, has_budget, bud);
      }
      __syncthreads();
      const int nj = min(PLAN_REFIT_THREADS, K - j0);
      if (mine)
        for (int j = 0; j < nj; j++)
          r += plan_before(t_cls[j], t_ret[j], t_cost[j], j0 + j, cls, s.x, s.y, k) ? 1 : 0;
    }
    if (mine) {
      rank[base + k] = r;
      if (r == 0) {
        best[g] = k;
        if (best_score) best_score[g] = s;
      }
    }
  }
  __syncthreads();   // the ranks, written to global memory by this workgroup, are read by it below
  const float inv_e = 1.0f / (float)E;
  for (int e = tid; e < H * nu; e += PLAN_REFIT_THREADS) {
    const int h = e / nu, u = e - h * nu;
    const float* col = plans + ((size_t)h * N + base) * nu + u;   // candidate k at col[k * nu]
    float sum = 0.0f;
    for (int k = 0; k < K; k++)
      if (rank[base + k] < E) sum += col[(size_t)k * nu];
    const float m = sum * inv_e;
    float dev = 0.0f;
    for (int k = 0; k < K; k++)
      if (rank[base + k] < E) {
        const float d = col[(size_t)k * nu] - m;
        dev += d * d;
      }
    const size_t o = ((size_t)h * G + g) * nu + u;
    mean[o] = m;
    sigma[o] = fmaxf(sigma_min, sqrtf(dev * inv_e));
  }
}

// mean[h] = mean[h + 1], the last row zero, every sigma = sigma_init; `next` is a second buffer (no lane reads what another
// writes), copied back by the caller.  One lane per element of [H][row], row = G * nu.
__global__ __launch_bounds__(256) void k_plan_shift(int H, int row, const float* __restrict__ mean, float* __restrict__ next,
                                                     float* __restrict__ sigma, float sigma_init) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)H * row;
  if (t >= total) return;
  next[t] = t + row < total ? mean[t + row] : 0.0f;
  sigma[t] = sigma_init;
}

// mean = 0, sigma = sigma_init for the groups with a non-zero byte of mask ([G]; nullptr: every group)
__global__ __launch_bounds__(256) void k_plan_clear(int H, int G, int nu, const uint8_t* __restrict__ mask, float* __restrict__ mean,
                                                     float* __restrict__ sigma, float sigma_init) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)H * G * nu;
  if (t >= total) return;
  const int g = (int)((t / nu) % G);
  if (mask && !mask[g]) return;
  mean[t] = 0.0f;
  sigma[t] = sigma_init;
}

}  // namespace sag

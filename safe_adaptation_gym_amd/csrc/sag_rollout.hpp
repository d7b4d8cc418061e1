// sag_rollout.hpp - what closes the rollout loop on the context stream after a device step, without a host decision:
//   k_episode_track    return / cost / length / goals met per env and the "ended" byte (sag_episode_track_device)
//   k_save_rows        the rows of the envs that ended, kept before the reset overwrites them (sag_copy_rows_device)
//   k_reset_commit     the install of a masked device reset, env by env (sag_reset_device_async)
//   k_observe_rows     Point / Car: the first observation of the new episodes, formed for the listed envs only
//   k_copy_rows        Doggo: the listed rows of a whole-batch observation
// The chain of a stream-ordered reset is k_reset_list -> k_reset_sample -> k_reset_commit -> observation.  The length of the
// list stays in device memory (n_dev); every launch is sized for n_envs and a block whose share of the list is empty
// returns at once.
#pragma once
#include "sag_reset.hpp"

namespace sag {

// One lane per env: 8 + 3 B and one float4 in, one byte and one float4 out, a second float4 for an env that ended.
// acc = {return, cost steps, length, goals met}; counts are exact in fp32 up to 2^24 steps.
__global__ __launch_bounds__(256) void k_episode_track(int N, const float* __restrict__ reward, const uint8_t* __restrict__ cost,
                                                        const uint8_t* __restrict__ done, const uint8_t* __restrict__ met, int max_steps,
                                                        float4* __restrict__ acc, uint8_t* __restrict__ ended, float4* __restrict__ episode) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float4 a = acc[i];
  a.x += reinterpret_cast<const float2*>(reward)[i].x;
  a.y += cost[i] != 0 ? 1.0f : 0.0f;
  a.z += 1.0f;
  a.w += met[i] != 0 ? 1.0f : 0.0f;
  const int e = done[i] ? 1 : (max_steps > 0 && a.z >= (float)max_steps ? 2 : 0);
  ended[i] = (uint8_t)e;
  if (e) {
    episode[i] = a;
    a = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  acc[i] = a;
}

__global__ __launch_bounds__(256) void k_episode_clear(int N, const uint8_t* __restrict__ mask, float4* __restrict__ acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N && mask[i]) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// For the envs with a non-zero mask byte (mask == nullptr: every env), row i of src -> row i of dst, Q float4 pieces each.
// One wavefront per 64 consecutive envs.  A wavefront whose 64 mask bytes are zero has read them and nothing else.  Otherwise
// the set lanes write their lane numbers to tab[] in rank order and all 64 lanes walk the count * Q pieces of those rows:
// piece p is piece p % Q of the row of tab[p / Q] - kept per lane as (e, q) = (p / Q, p % Q) and advanced by 64 pieces at a
// time, so no product can overflow for any row size.  Under a full mask tab[e] = e and consecutive lanes touch consecutive 16
// bytes of one 64-row span.  SAVE_PIECES pieces per lane are loaded before the first is stored: with 32 wavefronts per CU
// that is 128 KiB in flight per CU, where one piece per lane (32 KiB) would not cover the memory latency at the copy rate.
constexpr int SAVE_PIECES = 4;
__global__ __launch_bounds__(WAVE) void k_save_rows(int N, const uint8_t* __restrict__ mask, int Q, const float4* __restrict__ src,
                                                     float4* __restrict__ dst) {
  __shared__ int tab[WAVE];
  const int lane = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * WAVE, i = row0 + lane;
  const bool set = i < (size_t)N && (!mask || mask[i] != 0);
  const uint64_t b = __ballot(set);
  if (b == 0) return;
  if (set) tab[__popcll(b & ((1ull << lane) - 1))] = lane;
  __syncthreads();
  const int count = __popcll(b), de = WAVE / Q, dq = WAVE % Q;
  int e = lane / Q, q = lane % Q;
  while (e < count) {
    size_t at[SAVE_PIECES];
    int n = 0;   // pieces of this pass that exist for this lane
#pragma unroll
    for (int u = 0; u < SAVE_PIECES; u++) {
      if (e < count) n = u + 1;
      at[u] = (row0 + (size_t)tab[min(e, count - 1)]) * (size_t)Q + (size_t)q;
      e += de;
      q += dq;
      if (q >= Q) { q -= Q; e++; }
    }
    if (n == SAVE_PIECES) {   // no branch between the loads: they are issued back to back, then the stores
      float4 v[SAVE_PIECES];
#pragma unroll
      for (int u = 0; u < SAVE_PIECES; u++) v[u] = src[at[u]];
#pragma unroll
      for (int u = 0; u < SAVE_PIECES; u++) dst[at[u]] = v[u];
    } else {                  // the lane's last pass
#pragma unroll
      for (int u = 0; u < SAVE_PIECES - 1; u++)
        if (u < n) dst[at[u]] = src[at[u]];
    }
  }
}

struct CommitArgs {
  float* S; int32_t* I; int32_t N;
  const int32_t* ids;           // the list of k_reset_list
  const int32_t* n_dev;         // its length
  const float* rec_f;           // staging records of k_reset_sample, record of ids[j] at j
  const int32_t* rec_i;
  const int32_t* status;        // [N] by env, written by k_reset_sample for every listed env
  uint8_t* cost;                // [N] cost bytes of the last host-buffer step (k_clear_cost)
  float* L_f; int32_t* L_i;     // layout store of sag_reset, by env
  float* hot; float* hot_haz;   // hot records (split form) or nullptr
  float4* acc;                  // episode accumulators or nullptr
  unsigned long long* totals;   // [0] envs reset, [1] envs whose sampling failed
};

// Per listed env whose sampling succeeded: k_install(init_task = 1), k_clear_cost, k_extract into the env's row of the layout
// store, its hot record, its episode accumulators.  An env whose sampling failed keeps everything and gets the
// ResamplingError bit (and a hot record that holds it).  One atomic per wavefront and counter.
__global__ __launch_bounds__(256) void k_reset_commit(CommitArgs p) {
  const int n = *p.n_dev;
  if ((int)(blockIdx.x * blockDim.x) >= n) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  bool ok = false, failed = false;
  if (j < n) {
    const int i = p.ids[j];
    ok = p.status[i] == 0;
    failed = !ok;
    if (ok) {
      install_env(p.S, p.I, p.N, i, p.rec_f + (size_t)j * SAG_REC_FLOATS, p.rec_i + (size_t)j * SAG_REC_INTS, 1);
      p.cost[i] = 0;
      extract_env(p.S, p.I, p.N, i, p.L_f + (size_t)i * SAG_REC_FLOATS, p.L_i + (size_t)i * SAG_REC_INTS);
      if (p.acc) p.acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      p.I[iaddr(DI_FLAGS, (size_t)p.N, (size_t)i)] |= 1;
    }
    if (p.hot) hot_refresh_env(p.S, p.I, p.N, (size_t)i, p.hot, p.hot_haz);
  }
  const uint64_t m_ok = __ballot(ok), m_failed = __ballot(failed);
  if (lane == 0 && m_ok) atomicAdd(p.totals, (unsigned long long)__popcll(m_ok));
  if (lane == 0 && m_failed) atomicAdd(p.totals + 1, (unsigned long long)__popcll(m_failed));
}

// Point / Car: step_body's observation over the list, as the busy kernel runs it over its rows (MODE_BUSY, state read from
// the group-major arrays), 64 list entries per wavefront; rows go straight into p.obs.  Entries whose sampling failed are
// skipped.  p.observe_only = 1, p.hot = nullptr.
template <int ROBOT, bool HAS_BTN, bool HAS_TBOX>
__global__ __launch_bounds__(WAVE, SAG_STEP_MIN_WAVES) void k_observe_rows(StepArgs p, const int32_t* ids, const int32_t* n_dev,
                                                                            const int32_t* status) {
  __shared__ float lds[LDS_FLOATS + (ROBOT == SAG_ROBOT_CAR ? CAR_PARK_SLOTS * WAVE : 0)];
  __shared__ int rows[WAVE];
  const int n = *n_dev, c0 = blockIdx.x * WAVE;
  if (c0 >= n) return;
  const int lane = threadIdx.x, nval = min(WAVE, n - c0);
  const int i = ids[c0 + (lane < nval ? lane : 0)];
  const bool live = lane < nval && status[i] == 0;
  const uint64_t skip = __ballot(!live);
  if (skip == ~0ull) return;
  rows[lane] = i;
  __syncthreads();
  step_body<ROBOT, HAS_BTN, HAS_TBOX, MODE_BUSY>(p, lds, lane, i, live, 0, nval, skip, rows);
}

// the rows of the listed envs whose sampling succeeded, src -> dst; one thread per (list entry, 16-byte piece)
__global__ __launch_bounds__(256) void k_copy_rows(const int32_t* ids, const int32_t* n_dev, const int32_t* status, int Q,
                                                    const float4* __restrict__ src, float4* __restrict__ dst) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)*n_dev * Q;
  if (t >= total) return;
  const int i = ids[t / Q];
  if (status[i] == 0) dst[(size_t)i * Q + t % Q] = src[(size_t)i * Q + t % Q];
}

}  // namespace sag

// sag_fork.hpp - env i of a destination context takes the complete state of env src[i] of a source context on the same
// GPU (sag_fork_device), on the destination's stream, without a host copy or a host wait.  The source may be the
// destination itself (a fork inside a batch) or a context with another n_envs (a few real envs feeding many planner envs;
// a context of the same size is a snapshot).
//   k_fork_decide   one lane per destination env: does it commit, and from which source; the two counters
//   k_fork_state    the 48 float4 groups of S, group-major: coalesced 16-byte stores, a 1 -> K broadcast reads one line
//   k_fork_rows     the env's row of the layout store (sag_reset then restarts the source's layout), 16 bytes per lane
//   k_fork_finish   the int words, the busy bits, accumulators, cost byte, descriptor index and the hot record
// Every launch is sized for the destination's n_envs; the decision stays on the device.
// Bytes per committed env: 768 (S) + 800 (layout row) + 20 (int words) + 16 (accumulators) + 1 + 4, read and written once
// each, + 384 of hot record where the context has them.
#pragma once
#include "sag_device.hpp"

namespace sag {

constexpr int FORK_GROUPS_PER_LANE = 8, FORK_CHUNKS = DEV_GROUPS / FORK_GROUPS_PER_LANE;
static_assert(DEV_GROUPS % FORK_GROUPS_PER_LANE == 0, "the groups divide into whole chunks");
constexpr int FORK_ROW_PIECES = SAG_REC_FLOATS / 4 + SAG_REC_INTS / 4;   // 16-byte pieces of one layout-store row

struct ForkArgs {
  float* S; int32_t* I; int32_t N;                              // destination
  const float* src_S; const int32_t* src_I; int32_t src_N;      // source (the destination's own arrays for a fork in place)
  const int32_t* src;            // [N] source env of every destination env, negative: keep
  int32_t* from;                 // [N] the decision: the source env of a committed env, else -1
  int32_t same_stream;           // SAG_FORK_SAME_STREAM: the env id travels with the state
  float* L_f; int32_t* L_i; const float* src_L_f; const int32_t* src_L_i;
  float4* acc; const float4* src_acc;                           // episode accumulators or nullptr
  uint8_t* cost; const uint8_t* src_cost;
  int32_t* desc_of_env; const int32_t* src_desc_of_env;         // both set or both nullptr
  float* hot; float* hot_haz;                                   // hot records of the destination or nullptr
  unsigned long long* totals;    // [0] envs copied, [1] envs rejected
};

// Env i commits if its source j = src[i] exists and - in one context - is not itself overwritten by this call: no committed
// read can then meet a committed write.  j == i is a copy onto itself.  One atomic per wavefront and counter.
__global__ __launch_bounds__(256) void k_fork_decide(ForkArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  bool ok = false, rejected = false;
  if (i < p.N) {
    const int j = p.src[i];
    if (j >= 0) {
      ok = j < p.src_N;
      if (ok && p.src_S == p.S && j != i) {
        const int jj = p.src[j];
        ok = jj < 0 || jj == j;
      }
      rejected = !ok;
    }
    p.from[i] = ok ? j : -1;
  }
  const uint64_t m_ok = __ballot(ok), m_rejected = __ballot(rejected);
  if (lane == 0 && m_ok) atomicAdd(p.totals, (unsigned long long)__popcll(m_ok));
  if (lane == 0 && m_rejected) atomicAdd(p.totals + 1, (unsigned long long)__popcll(m_rejected));
}

// Block b: envs (b / FORK_CHUNKS) * 256 .., groups (b % FORK_CHUNKS) * 8 ..; a lane loads its env's eight float4, then stores them
__global__ __launch_bounds__(256) void k_fork_state(ForkArgs p) {
  const size_t i = (size_t)(blockIdx.x / FORK_CHUNKS) * blockDim.x + threadIdx.x;
  const int g0 = (int)(blockIdx.x % FORK_CHUNKS) * FORK_GROUPS_PER_LANE;
  if (i >= (size_t)p.N) return;
  const int j = p.from[i];
  if (j < 0 || (p.src_S == p.S && (size_t)j == i)) return;
  const float4* __restrict__ A = reinterpret_cast<const float4*>(p.src_S);
  float4* __restrict__ B = reinterpret_cast<float4*>(p.S);
  const size_t Ns = (size_t)p.src_N, Nd = (size_t)p.N;
  float4 v[FORK_GROUPS_PER_LANE];
#pragma unroll
  for (int g = 0; g < FORK_GROUPS_PER_LANE; g++) v[g] = A[(size_t)(g0 + g) * Ns + (size_t)j];
#pragma unroll
  for (int g = 0; g < FORK_GROUPS_PER_LANE; g++) B[(size_t)(g0 + g) * Nd + i] = v[g];
}

// one lane per (env, 16-byte piece) of the AoS layout store: a row is 800 contiguous bytes on either side.  The row keeps
// its own SAG_I_ENV_ID unless the env id travels
__global__ __launch_bounds__(256) void k_fork_rows(ForkArgs p) {
  constexpr int QF = SAG_REC_FLOATS / 4, QI = SAG_REC_INTS / 4;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)p.N * FORK_ROW_PIECES) return;
  const size_t i = t / FORK_ROW_PIECES;
  const int q = (int)(t % FORK_ROW_PIECES);
  const int j = p.from[i];
  if (j < 0 || (p.src_S == p.S && (size_t)j == i)) return;
  if (q < QF) {
    reinterpret_cast<float4*>(p.L_f)[i * QF + q] = reinterpret_cast<const float4*>(p.src_L_f)[(size_t)j * QF + q];
  } else {
    int4 v = reinterpret_cast<const int4*>(p.src_L_i)[(size_t)j * QI + (q - QF)];
    if (!p.same_stream && q - QF == SAG_I_ENV_ID / 4) (&v.x)[SAG_I_ENV_ID % 4] = p.L_i[i * SAG_REC_INTS + SAG_I_ENV_ID];
    reinterpret_cast<int4*>(p.L_i)[i * QI + (q - QF)] = v;
  }
}

// One lane per env, after k_fork_state: the int4 word (with the env's own id unless it travels) and the tstate word with both
// copies of the busy bit set, as install_env leaves them - the first step of a copy runs in the busy kernel -; then what
// hangs on an env outside S and I, and its hot record from the state just written
__global__ __launch_bounds__(256) void k_fork_finish(ForkArgs p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.N) return;
  const int j = p.from[i];
  if (j < 0) return;
  const size_t Ns = (size_t)p.src_N, Nd = (size_t)p.N;
  const uint32_t busy = TS_BUSY_BIT | TS_BUSY_BIT << 1;
  if (p.src_S == p.S && (size_t)j == i) {
    p.I[iaddr(DI_TSTATE, Nd, i)] = (int32_t)((uint32_t)p.I[iaddr(DI_TSTATE, Nd, i)] | busy);
  } else {
    int4 iw = reinterpret_cast<const int4*>(p.src_I + ipad(Ns))[j];
    if (!p.same_stream) iw.z = p.I[iaddr(DI_ENVID, Nd, i)];
    reinterpret_cast<int4*>(p.I + ipad(Nd))[i] = iw;
    p.I[iaddr(DI_TSTATE, Nd, i)] = (int32_t)((uint32_t)p.src_I[iaddr(DI_TSTATE, Ns, (size_t)j)] | busy);
    if (p.acc) p.acc[i] = p.src_acc ? p.src_acc[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    p.cost[i] = p.src_cost[j];
    if (p.desc_of_env) p.desc_of_env[i] = p.src_desc_of_env[j];
  }
  if (p.hot) hot_refresh_env(p.S, p.I, p.N, i, p.hot, p.hot_haz);
}

}  // namespace sag

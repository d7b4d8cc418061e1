// sag_buffer.hpp - what a time-major rollout buffer needs on the context stream besides the step itself:
//   k_append_rows      the rows of the envs that ended, compacted into a store of `capacity` rows (sag_append_rows_device)
//   k_gae              advantages and returns of the reward and the cost channel over T stored steps (sag_gae_device)
#pragma once
#include "sag_rollout.hpp"

namespace sag {

// The compacting sibling of k_save_rows: one wavefront per 64 consecutive envs.  The wavefront claims count = popcount(ballot)
// consecutive slots with ONE returning atomic add (lane 0; the base is broadcast), so the set lane of rank e owns slot
// base + e: slots ascend with the env index inside a wavefront, and between wavefronts they come in the order the adds land.
// The counter keeps counting past `capacity`; a claim at or beyond it gets slot -1 and moves nothing.  Because the rows that fit
// are the first `fit` ranks and their slots are consecutive, the destination of the piece walk is one contiguous run of
// fit * Q pieces starting at slot `base`: piece p of the run is piece p % Q of the row of tab[p / Q], kept per lane as
// (e, q) and advanced by 64 pieces at a time exactly as in k_save_rows (no product can overflow for any row size).
// A wavefront whose 64 mask bytes are zero has read them and written its 64 slots of -1, nothing else.
__global__ __launch_bounds__(WAVE) void k_append_rows(int N, const uint8_t* __restrict__ mask, int Q, const float4* __restrict__ src,
                                                       float4* __restrict__ store, int capacity, int* __restrict__ counter,
                                                       int32_t* __restrict__ slot) {
  __shared__ int tab[WAVE];
  const int lane = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * WAVE, i = row0 + lane;
  const bool set = i < (size_t)N && mask[i] != 0;
  const uint64_t b = __ballot(set);
  if (b == 0) {
    if (i < (size_t)N) slot[i] = -1;
    return;
  }
  const int count = __popcll(b), rank = __popcll(b & ((1ull << lane) - 1));
  int base = 0;
  if (lane == 0) base = atomicAdd(counter, count);
  base = __shfl(base, 0);
  // (a counter that has wrapped past 2^31 claims is negative: nothing fits)
  const int fit = base < 0 ? 0 : min(count, max(capacity - base, 0));
  if (i < (size_t)N) slot[i] = set && rank < fit ? base + rank : -1;
  if (fit == 0) return;
  if (set) tab[rank] = lane;
  __syncthreads();
  const int de = WAVE / Q, dq = WAVE % Q;
  int e = lane / Q, q = lane % Q;
  size_t out = (size_t)base * (size_t)Q + (size_t)lane;   // the lane's piece of the destination run
  while (e < fit) {
    size_t at[SAVE_PIECES];
    int n = 0;   // pieces of this pass that exist for this lane
#pragma unroll
    for (int u = 0; u < SAVE_PIECES; u++) {
      if (e < fit) n = u + 1;
      at[u] = (row0 + (size_t)tab[min(e, fit - 1)]) * (size_t)Q + (size_t)q;
      e += de;
      q += dq;
      if (q >= Q) { q -= Q; e++; }
    }
    if (n == SAVE_PIECES) {   // no branch between the loads: they are issued back to back, then the stores
      float4 v[SAVE_PIECES];
#pragma unroll
      for (int u = 0; u < SAVE_PIECES; u++) v[u] = src[at[u]];
#pragma unroll
      for (int u = 0; u < SAVE_PIECES; u++) store[out + (size_t)u * WAVE] = v[u];
    } else {                  // the lane's last pass
#pragma unroll
      for (int u = 0; u < SAVE_PIECES - 1; u++)
        if (u < n) store[out + (size_t)u * WAVE] = src[at[u]];
    }
    out += (size_t)SAVE_PIECES * WAVE;
  }
}

// ---- generalised advantage estimation ------------------------------------------------------------------------------
// One lane per env walks t = T-1 ... 0.  Per step and channel only two multiply-add pairs are serial (q, s, delta; p, A, ret -
// every operation rounded on its own: the translation unit is built with -ffp-contract=off), and every load address but the
// final-value gather is known in advance.  So the loads of GAE_DEPTH steps are kept in flight ahead of the chain in a register
// ring: step t is consumed from ring[u] and the load of step t - GAE_DEPTH is issued into the same entry.  With both channels
// that is 8 steps * 22 B * 64 lanes = 11 KiB per wavefront - at 4096 envs, where one wavefront per CU is all there is, an HBM
// miss (~900 cycles) is paid once per 8 steps instead of once per step; at millions of envs occupancy alone streams.
// value[t + 1] of a step that did not end is the value the chain loaded one step earlier: each value row is read once.
constexpr int GAE_DEPTH = 8;

struct GaeArgs {
  int N, T, pitch, capacity;
  float gamma, gl, cgamma, cgl;   // gl = gamma * lam, rounded once on the host
  const float* reward; const uint8_t* cost; const uint8_t* ended;
  const float* value; const float* cvalue;
  const int32_t* slot; const float* final_value; const float* final_cvalue;
  float* adv; float* ret; float* cadv; float* cret;
};

struct GaeStep { float r, v, cv; int32_t slot; uint8_t c, e; };

// Element `lane` of a plane: the plane's address is wave-uniform (scalar registers) and the lane's share is a 32-bit byte
// offset, so a load or store needs no 64-bit address of its own in vector registers - with 8 steps of 6 arrays in flight those
// addresses, not the data, would set the register count.  (The byte offset of the widest row, 8 * i, must fit 32 bits:
// sag_gae_device refuses contexts of 2^28 envs or more.)
template <class T>
__device__ __forceinline__ const T& gae_at(const T* plane, uint32_t lane_bytes) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(plane) + lane_bytes);
}
template <class T>
__device__ __forceinline__ T& gae_at(T* plane, uint32_t lane_bytes) {
  return *reinterpret_cast<T*>(reinterpret_cast<char*>(plane) + lane_bytes);
}

// row = t * pitch, the step's plane in elements (wave-uniform); i = the lane's env
template <bool COST, bool SLOT>
__device__ __forceinline__ void gae_load(const GaeArgs& p, size_t row, uint32_t i, GaeStep& s) {
  s.r = gae_at(p.reward + 2 * row, 8u * i);
  s.e = gae_at(p.ended + row, i);
  s.v = gae_at(p.value + row, 4u * i);
  if (COST) { s.c = gae_at(p.cost + row, i); s.cv = gae_at(p.cvalue + row, 4u * i); }
  if (SLOT) s.slot = gae_at(p.slot + row, 4u * i);
}

// one step of one channel: r, the value of the next state (already chosen), this step's value; carry in and out
__device__ __forceinline__ void gae_channel(float gamma, float gl, float r, float nv, float v, float& carry, float& A, float& ret) {
  const float q = gamma * nv;
  const float s = r + q;
  const float delta = s - v;
  const float pr = gl * carry;
  A = delta + pr;
  ret = A + v;
  carry = A;
}

template <bool COST, bool SLOT>
__device__ __forceinline__ void gae_consume(const GaeArgs& p, size_t row, uint32_t i, const GaeStep& s, float& vnext, float& cvnext,
                                            float& carry, float& ccarry) {
  float nv = vnext, cnv = cvnext;
  if (s.e != 0) {   // the episode ended here: value[t + 1] belongs to the next one
    nv = 0.0f; cnv = 0.0f; carry = 0.0f; ccarry = 0.0f;
    if (SLOT && s.e == 2 && s.slot >= 0 && s.slot < p.capacity) {   // truncated, and its final row was kept: the one dependent load
      if (p.final_value) nv = p.final_value[s.slot];
      if (COST && p.final_cvalue) cnv = p.final_cvalue[s.slot];
    }
  }
  float A, ret;
  gae_channel(p.gamma, p.gl, s.r, nv, s.v, carry, A, ret);
  gae_at(p.adv + row, 4u * i) = A;
  gae_at(p.ret + row, 4u * i) = ret;
  vnext = s.v;
  if (COST) {
    gae_channel(p.cgamma, p.cgl, s.c != 0 ? 1.0f : 0.0f, cnv, s.cv, ccarry, A, ret);
    gae_at(p.cadv + row, 4u * i) = A;
    gae_at(p.cret + row, 4u * i) = ret;
    cvnext = s.cv;
  }
}

template <bool COST, bool SLOT>
__global__ __launch_bounds__(WAVE) void k_gae(GaeArgs p) {
  const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= (uint32_t)p.N) return;
  const size_t P = (size_t)p.pitch, back = (size_t)GAE_DEPTH * P;
  GaeStep ring[GAE_DEPTH];
  int t = p.T - 1;
  float vnext = gae_at(p.value + (size_t)p.T * P, 4u * i), cvnext = COST ? gae_at(p.cvalue + (size_t)p.T * P, 4u * i) : 0.0f;
  float carry = 0.0f, ccarry = 0.0f;
#pragma unroll
  for (int u = 0; u < GAE_DEPTH; u++) gae_load<COST, SLOT>(p, (size_t)max(t - u, 0) * P, i, ring[u]);   // (T < depth: step 0 again, unused)
  while (t >= 2 * GAE_DEPTH - 1) {   // every step of the pass exists and so does every step it loads: no branch between the loads
#pragma unroll
    for (int u = 0; u < GAE_DEPTH; u++) {
      const size_t row = (size_t)(t - u) * P;
      gae_consume<COST, SLOT>(p, row, i, ring[u], vnext, cvnext, carry, ccarry);
      gae_load<COST, SLOT>(p, row - back, i, ring[u]);
    }
    t -= GAE_DEPTH;
  }
  for (int pass = 0; pass < 2; pass++) {   // the last 2 * depth - 1 steps at most
#pragma unroll
    for (int u = 0; u < GAE_DEPTH; u++) {
      const int tt = t - u;
      if (tt >= 0) {
        const size_t row = (size_t)tt * P;
        gae_consume<COST, SLOT>(p, row, i, ring[u], vnext, cvnext, carry, ccarry);
        if (tt >= GAE_DEPTH) gae_load<COST, SLOT>(p, row - back, i, ring[u]);
      }
    }
    t -= GAE_DEPTH;
  }
}

}  // namespace sag

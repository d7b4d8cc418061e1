// sag_shuffle.hpp - a random permutation of [0, n) written on the device (sag_permutation_device; include/sag.h defines it bit
// for bit): the row list a learner hands to sag_policy_backward_rows_device once per epoch, with no upload and no sort.
//   k_permutation      one lane per position i: pi(i) by a keyed Feistel network on the next power of two, walked until the
//                      value falls below n (cycle walking); one 4-byte vector store per lane, no atomics, no workspace
// pi is a keyed pseudo-random permutation, not a uniform draw from all n! orders: a key and a draw select one of at most 2^96
// of them.  Over the draws the position x value table of n = 130 is flat (max |z| 4.4, chi^2 / dof 1.015 over 16384 draws,
// one standard deviation of that ratio being 0.011; tests/test_shuffle_ref.py).  Below about 16 elements the halves of the
// network are 1 to 2 bits wide and the distribution is visibly non-uniform (n = 5: chi^2 / dof 7 to 9; n = 13: 1.19): at those
// sizes the function promises a bijection and nothing more.  A learner's T x N is never that small.
#pragma once
#include "sag_device.hpp"

namespace sag {

// Counter word 3 of the permutation's draws: stream 6, placed as streams 4 (the planner, sag_plan.hpp) and 5 (the policy) are -
// in the bits above the 26 (episode nonce << 2 | stream) that streams 0 - 3 use.
constexpr uint32_t SHUFFLE_STREAM_WORD = 6u << 26;
constexpr int SHUFFLE_ROUNDS = 6;   // even: the halves end at the widths they started with (4 rounds: chi^2 / dof 2.8 at n = 13)
constexpr int SHUFFLE_THREADS = 256;

// the walk domain is 2^b: b = max(2, bit length of n - 1), so n <= 2^b and, for n > 2, 2^b < 2 n
inline int shuffle_bits(int32_t n) {
  int b = 0;
  for (uint32_t m = (uint32_t)(n - 1); m; m >>= 1) b++;
  return b < 2 ? 2 : b;
}

// F: an unbalanced Feistel network on b-bit words (b <= 31), a bijection of [0, 2^b) whatever the round function returns
__device__ inline uint32_t shuffle_feistel(uint32_t x, int b, uint32_t draw, uint32_t k0, uint32_t k1) {
  int wl = b >> 1, wr = b - wl;
  uint32_t L = x >> wr, R = x & ((1u << wr) - 1u);
#pragma unroll
  for (int r = 0; r < SHUFFLE_ROUNDS; r++) {
    uint32_t c[4] = {R, draw, (uint32_t)r, SHUFFLE_STREAM_WORD};
    philox4x32_10(c, k0, k1);
    const uint32_t t = L ^ (c[0] & ((1u << wl) - 1u));
    L = R; R = t;
    const int w = wl; wl = wr; wr = w;
  }
  return (L << wr) | R;
}

// index[i] = pi(i): x = i; do x = F(x) while x >= n.  The walk ends because F permutes [0, 2^b) and i < n lies on a cycle that
// returns to [0, n); its expected length is 2^b / n < 2 rounds.
__global__ __launch_bounds__(SHUFFLE_THREADS) void k_permutation(uint32_t n, int b, uint32_t draw, uint32_t k0, uint32_t k1,
                                                                  int32_t* __restrict__ index) {
  const uint32_t i = blockIdx.x * (uint32_t)SHUFFLE_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t x = i;
  do x = shuffle_feistel(x, b, draw, k0, k1); while (x >= n);
  index[i] = (int32_t)x;
}

}  // namespace sag

"""NumPy restatement of sag_permutation_device (include/sag.h defines pi; csrc/sag_shuffle.hpp computes it): a 6-round
unbalanced Feistel network on the next power of two, keyed by Philox4x32-10 (reset_sampler_ref.philox) under the context key
and `draw`, walked until the value falls below n.  test_shuffle_ref.py pins it on its own; the device is compared with it bit
for bit (test_shuffle.py)."""
import numpy as np

from reset_sampler_ref import philox

STREAM_WORD = 0x18000000   # counter word 3: stream 6, beside the planner's 0x10000000 and the policy's 0x14000000
ROUNDS = 6


def bits(n):
  """b = max(2, bit length of n - 1): the walk domain is 2^b."""
  return max(2, int(n - 1).bit_length())


def feistel(x, b, draw, key, rounds=ROUNDS):
  """F(x) for an array of b-bit words -> uint32 array.  `key`: the 64-bit context key."""
  k0, k1 = key & 0xffffffff, (key >> 32) & 0xffffffff
  wl = b // 2
  wr = b - wl
  x = np.asarray(x, np.uint32)
  L, R = x >> np.uint32(wr), x & np.uint32((1 << wr) - 1)
  for r in range(rounds):
    f = philox(R, draw & 0xffffffff, r, STREAM_WORD, k0, k1)[0] & np.uint32((1 << wl) - 1)
    L, R = R, L ^ f
    wl, wr = wr, wl
  return (L << np.uint32(wr)) | R


def permutation(n, draw, key, rounds=ROUNDS, walks=None):
  """pi(0 ... n - 1) as int32: x = i; do x = F(x) while x >= n.  walks: a list that receives the number of rounds of the longest
  walk."""
  return permutations(n, [draw], key, rounds, walks)[0]


def permutations(n, draws, key, rounds=ROUNDS, walks=None):
  """[len(draws), n] int32: row d is pi under draws[d] (all walks advance together)."""
  n = int(n)
  b = bits(n)
  draws = np.asarray(draws, np.int64)
  x = np.tile(np.arange(n, dtype=np.uint32), len(draws))
  d = np.repeat(draws & 0xffffffff, n)
  todo = np.arange(x.size)
  longest = 0
  while todo.size:
    longest += 1
    x[todo] = feistel(x[todo], b, d[todo], key, rounds)
    todo = todo[x[todo] >= n]
  if walks is not None:
    walks.append(longest)
  return x.astype(np.int32).reshape(len(draws), n)


def table(n, draws, key, rounds=ROUNDS):
  """counts[i, v] = the draws d in `draws` with pi_d(i) == v."""
  p = permutations(n, draws, key, rounds)
  flat = (np.arange(n)[None, :] * n + p).reshape(-1)
  return np.bincount(flat, minlength=n * n).reshape(n, n)


def flatness(counts):
  """(max |z|, chi^2 / dof) of a position x value table against the uniform one: cell mean D / n, cell variance
  D / n (1 - 1 / n), (n - 1)^2 degrees of freedom (every row and every column sums to D)."""
  n = counts.shape[0]
  D = counts[0].sum()
  e = D / n
  z = (counts - e) / np.sqrt(e * (1 - 1 / n))
  chi2 = ((counts - e) ** 2 / e).sum()
  return float(np.abs(z).max()), float(chi2 / (n - 1) ** 2)

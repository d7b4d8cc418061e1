"""NumPy restatements of the rollout-buffer kernels (csrc/sag_buffer.hpp; contracts in include/sag.h).

  append_ref   what sag_append_rows_device may produce, as checks on its outputs (the order between wavefronts is free)
  gae_ref32    sag_gae_device's recipe with np.float32 scalars, one operation per line: the kernel equals it bit for bit
  gae_ref64    the textbook recurrence in float64, against which gae_ref32 itself is checked"""
import numpy as np

F = np.float32


def append_ref(mask, src, fill, capacity, c0, store, slot, count):
  """Asserts everything the header promises about one sag_append_rows_device call: mask [n] u8, src [n, row] u8, `fill` the
  store before the call ([capacity, row] u8), c0 the counter before it; store, slot, count what the call left.  Returns the
  number of rows written."""
  n = len(mask)
  on = np.flatnonzero(mask != 0)
  k = len(on)
  assert count == c0 + k, f'count {count}, expected {c0} + {k}'
  assert slot.shape == (n,) and slot.dtype == np.int32
  np.testing.assert_array_equal(slot[mask == 0], -1, err_msg='slot of an env outside the mask')
  got = slot[on]
  fit = max(0, min(k, capacity - c0))
  kept = got[got >= 0]
  assert len(kept) == fit, f'{len(kept)} rows have a slot, {fit} fit'
  # the claimed slots are c0 ... c0 + k - 1; those below capacity are handed out, each once
  np.testing.assert_array_equal(np.sort(kept), np.arange(c0, c0 + fit), err_msg='the slots handed out')
  # inside an aligned group of 64 envs the claim is one run: slots ascend with the env index, and a group that overflows keeps
  # its first ranks
  for g0 in range(0, n, 64):
    s = slot[g0:g0 + 64][mask[g0:g0 + 64] != 0]
    if len(s):
      ok = s >= 0
      assert not (ok[1:] & ~ok[:-1]).any(), f'group {g0 // 64}: a later rank fits where an earlier one did not'
      np.testing.assert_array_equal(s[ok], s[ok][0] + np.arange(ok.sum()) if ok.any() else s[ok], err_msg=f'group {g0 // 64}: one ascending run')
  for i in on:
    if slot[i] >= 0:
      np.testing.assert_array_equal(store[slot[i]], src[i], err_msg=f'env {i} -> slot {slot[i]}')
  untouched = np.ones(capacity, bool)
  untouched[kept] = False
  np.testing.assert_array_equal(store[untouched], fill[untouched], err_msg='rows of the store that no claim reached')
  return fit


def gae_ref32(reward, cost, ended, value, gamma, lam, slot=None, final_value=None, capacity=0, is_cost=False):
  """One channel.  reward [T, n] f32 (ignored for the cost channel, which takes r = cost != 0), ended [T, n] u8, value
  [T + 1, n] f32 -> (adv, ret) [T, n] f32."""
  T, n = ended.shape
  adv, ret = np.zeros((T, n), F), np.zeros((T, n), F)
  gamma = F(gamma)
  gl = F(gamma * F(lam))
  with np.errstate(all='ignore'):
    for i in range(n):
      carry = F(0)
      for t in range(T - 1, -1, -1):
        e = int(ended[t, i])
        if e == 0:
          nv = F(value[t + 1, i])
        elif e == 2 and slot is not None and final_value is not None and 0 <= int(slot[t, i]) < capacity:
          nv = F(final_value[int(slot[t, i])])
          carry = F(0)
        else:
          nv = F(0)
          carry = F(0)
        r = (F(1) if cost[t, i] != 0 else F(0)) if is_cost else F(reward[t, i])
        v = F(value[t, i])
        q = F(gamma * nv)
        s = F(r + q)
        delta = F(s - v)
        p = F(gl * carry)
        A = F(delta + p)
        rt = F(A + v)
        adv[t, i] = A
        ret[t, i] = rt
        carry = A
  return adv, ret


def gae_ref32_batch(reward, cost, ended, value, gamma, lam, slot=None, final_value=None, capacity=0, is_cost=False):
  """gae_ref32 with the envs side by side in float32 arrays: the same operations in the same order, each a NumPy ufunc of its
  own (so each is rounded on its own).  For the many-trajectory check of the recipe; the tests assert that the two agree bit
  for bit."""
  T, n = ended.shape
  adv, ret = np.zeros((T, n), F), np.zeros((T, n), F)
  gamma = F(gamma)
  gl = F(gamma * F(lam))
  carry = np.zeros(n, F)
  value = np.asarray(value, F)
  with np.errstate(all='ignore'):
    for t in range(T - 1, -1, -1):
      e = ended[t]
      nv = np.where(e == 0, value[t + 1], F(0))
      if slot is not None and final_value is not None:
        kept = (e == 2) & (slot[t] >= 0) & (slot[t] < capacity)
        nv = np.where(kept, np.asarray(final_value, F)[np.clip(slot[t], 0, capacity - 1)], nv)
      carry = np.where(e == 0, carry, F(0))
      r = (cost[t] != 0).astype(F) if is_cost else np.asarray(reward[t], F)
      v = value[t]
      q = gamma * nv
      s = r + q
      delta = s - v
      p = gl * carry
      A = delta + p
      rt = A + v
      assert q.dtype == s.dtype == delta.dtype == p.dtype == A.dtype == rt.dtype == F
      adv[t], ret[t], carry = A, rt, A
  return adv, ret


def gae_ref64(r, ended, value, gamma, lam, boot=None):
  """The textbook recurrence in float64, vectorised over envs: r [T, n], ended [T, n] (0, 1, 2), value [T + 1, n], boot [T, n]
  the bootstrap value of a truncated step (None: 0).  delta_t = r_t + gamma * V_next - V_t, A_t = delta_t + gamma * lam * A_{t+1},
  the chain cut where an episode ended."""
  r, value = np.asarray(r, np.float64), np.asarray(value, np.float64)
  T, n = ended.shape
  adv = np.zeros((T, n))
  carry = np.zeros(n)
  for t in range(T - 1, -1, -1):
    e = ended[t]
    nv = np.where(e == 0, value[t + 1], 0.0)
    if boot is not None:
      nv = np.where(e == 2, np.asarray(boot[t], np.float64), nv)
    carry = np.where(e == 0, carry, 0.0)
    adv[t] = r[t] + gamma * nv - value[t] + gamma * lam * carry
    carry = adv[t]
  return adv, adv + value[:-1]

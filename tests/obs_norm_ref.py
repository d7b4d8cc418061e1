"""NumPy restatements of the observation normalisation of include/sag.h (sag_obs_stats_device and the staging arithmetic of
sag_policy_forward_norm_device / sag_policy_backward_norm_device), written from the header's prose and independent of the kernels.

  normalize32      float32, every operation rounded on its own: the kernels equal it bit for bit
  batch_moments    (n_b, mean_b, M2_b) per column of a batch [rows, obs_dim], in float64 (the reference) or in float32 the way a
                   plain implementation sums - one row after the other, the header's shifted second pass - whose distance from the
                   float64 one is the error the device is granted 8 times
  merge            Chan et al. in float64, the header's association
  table32          the table of a state, bit for bit what the device writes
  measure          the errors of a state against the float64 one, per column on its natural scale, the largest over the columns

A state is the float64 array {count, mean[obs_dim], M2[obs_dim]}."""
import numpy as np

F32, F64 = np.float32, np.float64


def normalize32(x, table, clip):
  """x [..., obs_dim] float32, table [2, obs_dim] float32 (mean, rstd): fl(fl(x - mean) * rstd) clamped to +-clip; a NaN stays."""
  x, table, c = np.asarray(x, F32), np.asarray(table, F32), F32(clip)
  with np.errstate(invalid='ignore', over='ignore'):
    d = (x - table[0]).astype(F32)
    xh = (d * table[1]).astype(F32)
    xh = np.where(xh < -c, -c, xh)     # a NaN compares false twice and passes
    xh = np.where(xh > c, c, xh)
  return xh.astype(F32)


def batch_moments(x, dtype=F64):
  """x [rows, obs_dim] -> (n_b, mean_b [obs_dim] float64, M2_b [obs_dim] float64).  float64: the plain two-pass definition.
  float32: column sums one row after the other in float32, mean_b = sum / n_b in float64, s = float32(mean_b), the second pass
  sums fl(fl(x - s)^2) the same way, and M2_b = max(0, sum - n_b (mean_b - s)^2)."""
  x = np.asarray(x)
  n = x.shape[0]
  if np.dtype(dtype) == np.dtype(F64):
    x = x.astype(F64)
    mean = x.sum(axis=0) / n
    return float(n), mean, ((x - mean)**2).sum(axis=0)
  x = x.astype(F32)
  mean = np.cumsum(x, axis=0, dtype=F32)[-1].astype(F64) / F64(n)
  s = mean.astype(F32)
  d = (x - s).astype(F32)
  sq = np.cumsum((d * d).astype(F32), axis=0, dtype=F32)[-1].astype(F64)
  return float(n), mean, np.maximum(0.0, sq - F64(n) * (mean - s.astype(F64))**2)


def empty_state(obs_dim):
  return np.zeros(1 + 2 * obs_dim, F64)


def merge(state, batch):
  """The state after a batch (n_b, mean_b, M2_b): n = n_a + n_b, w = n_b / n, delta = mean_b - mean_a,
  mean = mean_a + delta w, M2 = (M2_a + M2_b) + delta^2 (n_a w)."""
  state = np.asarray(state, F64)
  od = (state.size - 1) // 2
  n_a, mean_a, M2_a = state[0], state[1:1 + od], state[1 + od:]
  n_b, mean_b, M2_b = batch
  n = n_a + F64(n_b)
  w = F64(n_b) / n
  delta = np.asarray(mean_b, F64) - mean_a
  return np.concatenate([[n], mean_a + delta * w, (M2_a + np.asarray(M2_b, F64)) + (delta * delta) * (n_a * w)])


def table32(state, eps):
  """[2, obs_dim] float32: mean = float32(mean), rstd = float32(1 / sqrt(M2 / n + float64(float32(eps)))); the identity (0, 1)
  while count is not above 0.  float64 sqrt and division are correctly rounded in NumPy as on the device."""
  state = np.asarray(state, F64)
  od = (state.size - 1) // 2
  n = state[0]
  if not n > 0:
    return np.stack([np.zeros(od, F32), np.ones(od, F32)])
  var = state[1 + od:] / n
  return np.stack([state[1:1 + od].astype(F32), (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)])


def resolved(ref):
  """The columns of a float64 state that measure() can judge: std >= 2^-10 |mean|, or std == 0 exactly (measure() then takes
  the mean's own scale and M2's absolute error).  A column with 0 < std < 2^-10 |mean| - constant in every batch, its M2 the
  rounding noise of the means, some (2^-24 |mean|)^2 per row in any float32 implementation and in none the same - is judged by
  near_constant_ok, not by a relative error of that noise."""
  ref = np.asarray(ref, F64)
  od = (ref.size - 1) // 2
  std, am = np.sqrt(ref[1 + od:] / ref[0]), np.abs(ref[1:1 + od])
  return (std >= 2.0**-10 * am) | (std == 0)


def near_constant_ok(state, ref):
  """The columns outside resolved(ref): the mean within n 2^-24 |mean| of the reference (the bound of a float32 sum of n terms
  of one sign, whatever the order) and the deviation within the same distance of the reference's."""
  state, ref = np.asarray(state, F64), np.asarray(ref, F64)
  od = (ref.size - 1) // 2
  n = ref[0]
  cols = ~resolved(ref)
  bound = n * 2.0**-24 * np.abs(ref[1:1 + od])
  mean_ok = np.abs(state[1:1 + od] - ref[1:1 + od]) <= bound
  std_ok = np.abs(np.sqrt(state[1 + od:] / state[0]) - np.sqrt(ref[1 + od:] / n)) <= bound
  return bool((mean_ok & std_ok)[cols].all())


def measure(state, ref, cols=None):
  """The largest error over the columns (all, or those of the mask `cols`) of a state against the float64 reference state: the
  mean's on the scale of the column's deviation (the mean's own where the deviation is 0), M2's relative."""
  state, ref = np.asarray(state, F64), np.asarray(ref, F64)
  od = (ref.size - 1) // 2
  n = ref[0]
  std = np.sqrt(ref[1 + od:] / n)
  am = np.abs(ref[1:1 + od])
  scale = np.where(std > 0, std, np.where(am > 0, am, 1.0))
  m2 = np.where(ref[1 + od:] > 0, ref[1 + od:], 1.0)
  em, e2 = np.abs(state[1:1 + od] - ref[1:1 + od]) / scale, np.abs(state[1 + od:] - ref[1 + od:]) / m2
  if cols is not None:
    em, e2 = em[cols], e2[cols]
  return dict(mean=float(em.max()), M2=float(e2.max()))

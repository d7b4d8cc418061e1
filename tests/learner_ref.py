"""NumPy restatements of the four learner functions of include/sag.h (sag_moments_device, sag_advantage_mix_device,
sag_lagrange_device, sag_grad_clip_device), written from the header's prose and independent of the kernels.

  moments64 / clip64   float64: what the two reductions are measured against
  moments32 / clip32   float32, the terms added one by one in storage order (np.cumsum): its distance from the float64 one
                       is the error a plain fp32 implementation makes on that input, and 8 times it is what the device is granted
  mix32, lagrange32    float32 with every operation rounded on its own: the device equals them bit for bit

`x` is the array of the elements that count, already selected (select() does it for a pitched, strided, masked array)."""
import numpy as np

F32, F64 = np.float32, np.float64


def select(x, n_rows, n_planes, pitch, stride=1, mask=None):
  """The counting elements of a device array in logical order: x holds n_planes * pitch * stride floats (or more), element
  (p, r) at (p * pitch + r) * stride; mask [n_planes * pitch] u8 or None."""
  flat = np.asarray(x).reshape(-1)
  idx = (np.arange(n_planes)[:, None] * pitch + np.arange(n_rows)[None, :]).reshape(-1)
  if mask is not None:
    idx = idx[np.asarray(mask).reshape(-1)[idx] != 0]
  return flat[idx * stride]


def moments64(x, eps):
  """-> [count, mean, var, rstd] in float64; eps is the float32 the device is given."""
  x = np.asarray(x, F64)
  n = x.size
  if n == 0:
    return np.zeros(4, F64)
  mean = x.sum() / n
  var = ((x - mean)**2).sum() / n
  return np.array([n, mean, var, 1.0 / (np.sqrt(var) + F64(F32(eps)))], F64)


def _seq_sum32(v):
  v = np.asarray(v, F32)
  return np.cumsum(v, dtype=F32)[-1] if v.size else F32(0)


def moments32(x, eps):
  """The same in float32: both sums one element after the other, the second pass on the float32 mean of the first."""
  x = np.asarray(x, F32)
  n = x.size
  if n == 0:
    return np.zeros(4, F32)
  cnt = F32(n)
  mean = F32(_seq_sum32(x) / cnt)
  d = (x - mean).astype(F32)
  var = F32(_seq_sum32((d * d).astype(F32)) / cnt)
  rstd = F32(F32(1) / F32(np.sqrt(var) + F32(eps)))
  return np.array([cnt, mean, var, rstd], F32)


def moments_measure(got, ref64):
  """The three errors of a moments array against the float64 one, each on its natural scale: the mean's on the deviation's
  (or the mean's own where the deviation is 0), var's and rstd's relative."""
  got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
  std = np.sqrt(ref64[2])
  scale = std if std > 0 else (abs(ref64[1]) if ref64[1] != 0 else 1.0)
  return dict(mean=abs(got[1] - ref64[1]) / scale, var=abs(got[2] - ref64[2]) / (ref64[2] if ref64[2] > 0 else 1.0),
              rstd=abs(got[3] - ref64[3]) / (ref64[3] if ref64[3] > 0 else 1.0))


def _norm32(x, mode, m, s):
  x = np.asarray(x, F32)
  if mode >= 1:
    x = (x - F32(m)).astype(F32)
  if mode == 2:
    x = (x * F32(s)).astype(F32)
  return x


def mix32(adv, cadv=None, adv_mode=0, cadv_mode=0, adv_mom=None, cadv_mom=None, lam=0.0):
  """out = norm(adv) - lam * norm(cadv) (cadv None: norm(adv)); the moments arrays are [count, mean, var, rstd]."""
  a = _norm32(adv, adv_mode, adv_mom[1] if adv_mode else 0, adv_mom[3] if adv_mode else 1)
  if cadv is None:
    return a
  c = _norm32(cadv, cadv_mode, cadv_mom[1] if cadv_mode else 0, cadv_mom[3] if cadv_mode else 1)
  t = (F32(lam) * c).astype(F32)
  return (a - t).astype(F32)


def mix64(adv, cadv=None, adv_mode=0, cadv_mode=0, adv_mom=None, cadv_mom=None, lam=0.0):
  def norm(x, mode, mom):
    x = np.asarray(x, F64)
    if mode >= 1:
      x = x - F64(mom[1])
    if mode == 2:
      x = x * F64(mom[3])
    return x
  a = norm(adv, adv_mode, adv_mom)
  return a if cadv is None else a - F64(lam) * norm(cadv, cadv_mode, cadv_mom)


def lagrange32(state, mom, lr, budget, lambda_max=np.inf):
  """-> the new state [lambda, mean cost, episodes, updates] (float32) after one sag_lagrange_device call."""
  s = np.array(state, F32)
  if mom[0] > 0:
    mean = F32(mom[1])
    step = F32(F32(lr) * F32(mean - F32(budget)))
    t = F32(s[0] + step)
    t = t if t > 0 else F32(0)
    t = t if t < F32(lambda_max) else F32(lambda_max)
    s[:] = (t, mean, F32(mom[0]), F32(s[3] + F32(1)))
  else:
    s[2] = 0
  return s


def lagrange64(lam, mean, lr, budget, lambda_max=np.inf):
  return min(float(lambda_max), max(0.0, float(lam) + float(lr) * (float(mean) - float(budget))))


def clip64(g, max_norm):
  """-> (norm, factor) in float64, the clip_grad_norm_ convention."""
  norm = np.sqrt((np.asarray(g, F64)**2).sum())
  return norm, min(1.0, float(max_norm) / (norm + 1e-6))


def clip32(g, max_norm):
  """-> (norm, factor, clipped gradient) in float32, the squares added one by one."""
  g = np.asarray(g, F32)
  norm = F32(np.sqrt(_seq_sum32((g * g).astype(F32))))
  f = F32(F32(max_norm) / F32(norm + F32(1e-6)))
  factor = F32(1) if f > 1 else f
  return norm, factor, scale32(g, factor)


def scale32(g, factor):
  g = np.asarray(g, F32)
  return g.copy() if factor == 1 else (g * F32(factor)).astype(F32)

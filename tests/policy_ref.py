"""NumPy restatement of sag_policy_forward_device (include/sag.h), independent of the kernel:
  fma32          an exact fmaf on float32 arrays: float64 product (exact), TwoSum, round to odd, one cast
  forward_ref32  the header's chains - acc = bias; acc = fmaf(x[k], W[k][j], acc) for ascending k; activation - bit for bit
  forward_ref64  the same network in float64
  layer_bound    the dot-product error bound of one layer
  normals_ref    the policy's standard normals in float64 (test_plan._normals_ref's transform on stream 5)
  pack / unpack  the parameter dict <-> the ABI's contiguous float32 layout
NumPy only."""
import numpy as np

import reset_sampler_ref as R

F32 = np.float32
POLICY_WORD = 0x14000000   # counter word 3 of the policy's draws (include/sag.h)
KEYS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'std')
TANH_C = F32(2.88539008177792681472)   # 2 log2(e), rounded to fp32 as the kernel's constant


def fma32(a, b, c):
  """fmaf(a, b, c) on float32 arrays, exactly: the product of two float32 is exact in float64; s + err is the exact sum of
  product and addend (TwoSum); where err != 0 and s has an even last bit, s moves one step toward err (round to odd), after
  which the cast to float32 rounds as one rounding of the exact value would."""
  a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
  with np.errstate(all='ignore'):
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.atleast_1d(s).view(np.uint64) & np.uint64(1)).reshape(np.shape(s)) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def act32(x, activation):
  if activation == 'relu':
    return np.where(x > 0, x, F32(0)).astype(F32)
  with np.errstate(all='ignore'):
    e = np.exp2((TANH_C * x).astype(F32)).astype(F32)
    return (F32(1) - F32(2) * (F32(1) / (e + F32(1))).astype(F32)).astype(F32)


def _layer32(x, W, b):
  acc = np.broadcast_to(np.asarray(b, F32), (x.shape[0], W.shape[1])).copy()
  for k in range(W.shape[0]):
    acc = fma32(x[:, k:k + 1], W[k][None, :], acc)
  return acc


def forward_ref32(params, obs, activation='relu', hidden=False):
  """-> mean [n, nu], value [n], cost value [n] (hidden=True: also the two hidden activations) in float32."""
  x = np.asarray(obs, F32)
  h1 = act32(_layer32(x, params['W1'], params['b1']), activation)
  h2 = act32(_layer32(h1, params['W2'], params['b2']), activation)
  o = _layer32(h2, params['W3'], params['b3'])
  nu = o.shape[1] - 2
  out = (o[:, :nu], o[:, nu], o[:, nu + 1])
  return out + (h1, h2) if hidden else out


def act64(x, activation):
  return np.maximum(x, 0.0) if activation == 'relu' else np.tanh(x)


def forward_ref64(params, obs, activation='relu'):
  x = np.asarray(obs, np.float64)
  P = {k: np.asarray(v, np.float64) for k, v in params.items()}
  h1 = act64(x @ P['W1'] + P['b1'], activation)
  h2 = act64(h1 @ P['W2'] + P['b2'], activation)
  o = h2 @ P['W3'] + P['b3']
  nu = o.shape[1] - 2
  return o[:, :nu], o[:, nu], o[:, nu + 1]


def layer_bound(x, W, b):
  """|fl(chain) - exact| <= (K + 2) u (|b| + sum |x||w|), u = 2^-24: K fused steps, each one rounding (gamma_K <= (K + 2) u
  for K u < 0.01)."""
  x, W, b = (np.asarray(v, np.float64) for v in (x, W, b))
  return (W.shape[0] + 2) * 2.0**-24 * (np.abs(b)[None, :] + np.abs(x) @ np.abs(W))


def normals_ref(key, id0, n, draw, nu):
  """z [n, nu] float64: Philox block (id0 + row, draw, u / 4, POLICY_WORD) under the key; uniforms ((w >> 8) + 0.5) / 2^24 in
  fp32, then the Box-Muller transform in float64; u % 4 = 0, 1 from words 0, 1 and 2, 3 from words 2, 3."""
  u = np.arange(nu)
  ids = ((int(id0) + np.arange(n)) & 0xffffffff)[:, None] + 0 * u[None, :]
  w = R.philox(ids, draw, (u // 4)[None, :] + 0 * ids, POLICY_WORD, key & 0xffffffff, key >> 32)
  hi = (u % 4 >= 2)[None, :]
  wa, wb = np.where(hi, w[2], w[0]), np.where(hi, w[3], w[1])
  u1 = (((wa >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(1 / 16777216.0)).astype(np.float64)
  u2 = (((wb >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(1 / 16777216.0)).astype(np.float64)
  r = np.sqrt(-2.0 * np.log(u1))
  return np.where((u % 2 == 0)[None, :], r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2))


def shapes(obs_dim, nu, hidden):
  return {'W1': (obs_dim, hidden), 'b1': (hidden,), 'W2': (hidden, hidden), 'b2': (hidden,), 'W3': (hidden, nu + 2),
          'b3': (nu + 2,), 'std': (nu,)}


def random_params(rng, obs_dim, nu, hidden, scale=1.0):
  p = {}
  for k, s in shapes(obs_dim, nu, hidden).items():
    bound = scale / np.sqrt(s[0]) if k[0] == 'W' else 0.5
    p[k] = rng.uniform(-bound, bound, s).astype(F32)
  p['std'] = rng.uniform(0.3, 1.2, nu).astype(F32)
  return p


def pack(params):
  return np.concatenate([np.asarray(params[k], F32).reshape(-1) for k in KEYS])


def logp_const(std):
  """S = sum log(std) + nu * 0.5 * log(2 pi), rounded once."""
  std = np.asarray(std, np.float64)
  return float(F32(np.log(std).sum() + len(std) * 0.5 * np.log(2 * np.pi)))

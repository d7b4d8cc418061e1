"""The NumPy restatement of the policy forward (tests/policy_ref.py) before anything is compared with it bit for bit: its
fused multiply-add against libm's fmaf, and its float32 chains against the float64 network within the dot-product bound.
No GPU, no library."""
import ctypes

import numpy as np

import policy_ref as P

F32 = np.float32


def _libm_fmaf(a, b, c):
  libm = ctypes.CDLL('libm.so.6')
  libm.fmaf.restype = ctypes.c_float
  libm.fmaf.argtypes = [ctypes.c_float] * 3
  return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)


def _bits(x):
  return np.asarray(x, F32).view(np.uint32)


def test_fma32_equals_libm_fmaf_on_random_triples():
  rng = np.random.RandomState(11)
  n = 1000000
  a = (rng.standard_normal(n) * np.exp2(rng.randint(-20, 21, n))).astype(F32)
  b = (rng.standard_normal(n) * np.exp2(rng.randint(-20, 21, n))).astype(F32)
  c = (rng.standard_normal(n) * np.exp2(rng.randint(-30, 31, n))).astype(F32)
  # a third of the addends cancel the product to within a few ulps, a third are the rounded product's neighbours
  p = (a.astype(np.float64) * b).astype(F32)
  c[::3] = -p[::3]
  c[1::3] = np.nextafter(-p[1::3], F32(0))
  np.testing.assert_array_equal(_bits(P.fma32(a, b, c)), _bits(_libm_fmaf(a, b, c)))


def test_fma32_on_float32_midpoints_with_a_residue():
  """a * b = -+(64 - 2^-40) * 2^e exactly and c has an odd last bit at ulp 128 * 2^e: the float64 sum rounds to the exact float32
  midpoint c -+ 64 * 2^e and loses the residue, so a plain cast would tie to even - away from c -, while fmaf returns c."""
  a, b, c = [], [], []
  for e in range(-12, 13, 3):
    for m in (1, 3, 0x155555, 0x7ffffd):            # odd mantissa offsets: c = (2^23 + m) * 128 * 2^e
      for sa in (1.0, -1.0):
        for sc in (1.0, -1.0):
          a.append(sa * (8.0 + 2.0**-20) * 2.0**e); b.append(8.0 - 2.0**-20); c.append(sc * (2.0**23 + m) * 128.0 * 2.0**e)
  a, b, c = (np.array(x, np.float64) for x in (a, b, c))
  assert (a.astype(F32) == a).all() and (b.astype(F32) == b).all() and (c.astype(F32) == c).all()
  s = a * b + c                                      # rounded: the residue 2^-40 * 2^e is below the last bit of s
  assert (np.abs(s - c) == 64.0 * np.exp2(np.repeat(np.arange(-12, 13, 3), 16))).all()
  want = _libm_fmaf(a, b, c)
  np.testing.assert_array_equal(_bits(want), _bits(c))   # the residue pulls every sum back to c
  assert (s.astype(F32) != want).all()               # and double rounding gets every one of them wrong
  np.testing.assert_array_equal(_bits(P.fma32(a, b, c)), _bits(want))


def test_forward_ref32_within_the_dot_product_bound_of_float64():
  rng = np.random.RandomState(5)
  for od, nu, H, act in ((60, 2, 32, 'relu'), (72, 2, 96, 'relu'), (104, 12, 64, 'relu'), (60, 2, 64, 'tanh')):
    prm = P.random_params(rng, od, nu, H, scale=2.0)
    obs = rng.uniform(-2, 2, (37, od)).astype(F32)
    mean, v, cv, h1, h2 = P.forward_ref32(prm, obs, act, hidden=True)
    out = np.concatenate([mean, v[:, None], cv[:, None]], axis=1)
    # each layer against float64 fed the SAME (float32) layer inputs, before the activation
    for x, W, b, got in ((obs, 'W1', 'b1', h1), (h1, 'W2', 'b2', h2), (h2, 'W3', 'b3', out)):
      exact = x.astype(np.float64) @ prm[W].astype(np.float64) + prm[b].astype(np.float64)
      bound = P.layer_bound(x, prm[W], prm[b])
      if W != 'W3':
        if act == 'relu':
          exact, bound = np.maximum(exact, 0.0), bound   # relu is 1-Lipschitz and exact
        else:
          continue   # the tanh layers carry the error of exp2 and the reciprocal: measured in test_policy.py, not bounded here
      assert (np.abs(got.astype(np.float64) - exact) <= bound).all(), (od, H, W)
    m64, v64, c64 = P.forward_ref64(prm, obs, act)
    assert np.abs(mean - m64).max() < 1e-4 and np.abs(v - v64).max() < 1e-4 and np.abs(cv - c64).max() < 1e-4

"""tests/learner_ref.py pinned without a GPU: against np.mean / np.var / np.linalg.norm in float64, the mixing formula written
out, and a multiplier sequence worked by hand."""
import numpy as np

import learner_ref as R

F32, F64 = np.float32, np.float64


def test_select_skips_pad_rows_other_columns_and_masked_elements():
  n_rows, n_planes, pitch, stride = 5, 3, 7, 4
  x = np.full((n_planes, pitch, stride), np.nan, F32)
  x[:, :n_rows, 1] = np.arange(15, dtype=F32).reshape(3, 5)
  got = R.select(x.reshape(-1)[1:], n_rows, n_planes, pitch, stride)
  np.testing.assert_array_equal(got, np.arange(15, dtype=F32))
  mask = np.zeros((n_planes, pitch), np.uint8)
  mask[1, 2] = 9
  mask[2, 6] = 1   # a pad row's byte is never looked at
  np.testing.assert_array_equal(R.select(x.reshape(-1)[1:], n_rows, n_planes, pitch, stride, mask), [7.0])


def test_moments64_is_numpy_mean_and_var():
  x = np.random.RandomState(0).normal(3.0, 2.0, 1001)
  eps = 1e-3
  m = R.moments64(x, eps)
  assert m[0] == 1001
  np.testing.assert_allclose(m[1], np.mean(x), rtol=1e-14)
  np.testing.assert_allclose(m[2], np.var(x), rtol=1e-13)
  np.testing.assert_allclose(m[3], 1.0 / (np.std(x) + F64(F32(eps))), rtol=1e-13)
  np.testing.assert_array_equal(R.moments64(np.zeros(0), eps), np.zeros(4))
  np.testing.assert_array_equal(R.moments32(np.zeros(0), eps), np.zeros(4, F32))


def test_moments32_is_close_to_moments64_and_exact_on_small_integers():
  x = np.random.RandomState(1).normal(-1.0, 0.5, 4097).astype(F32)
  own = R.moments_measure(R.moments32(x, 1e-8), R.moments64(x, 1e-8))
  assert all(0 <= v < 1e-4 for v in own.values()), own
  k = np.random.RandomState(2).randint(-2, 3, 999).astype(F32)
  m = R.moments32(k, 1e-8)
  assert m[0] == 999 and m.dtype == F32
  np.testing.assert_allclose(F64(m[1]) * 999, k.astype(F64).sum(), atol=1e-3)
  c = R.moments32(np.full(77, 1.5, F32), 1e-8)
  assert c[1] == F32(1.5) and c[2] == 0 and c[3] == F32(F32(1) / F32(1e-8))


def test_mix_modes_against_the_formula_written_out():
  rng = np.random.RandomState(3)
  adv, cadv = rng.normal(size=64).astype(F32), rng.normal(2.0, 3.0, size=64).astype(F32)
  ma, mc = R.moments32(adv, 1e-8), R.moments32(cadv, 1e-8)
  lam = 0.37
  for am in range(3):
    for cm in range(3):
      want = (adv.astype(F64) - (ma[1] if am else 0)) * (ma[3] if am == 2 else 1) - F64(F32(lam)) * (
          (cadv.astype(F64) - (mc[1] if cm else 0)) * (mc[3] if cm == 2 else 1))
      np.testing.assert_allclose(R.mix64(adv, cadv, am, cm, ma, mc, F32(lam)), want, rtol=1e-15)
      got = R.mix32(adv, cadv, am, cm, ma, mc, lam)
      assert got.dtype == F32
      np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)
    np.testing.assert_array_equal(R.mix32(adv, None, am, 0, ma), R._norm32(adv, am, ma[1], ma[3]))
  np.testing.assert_array_equal(R.mix32(adv), adv)
  s = R.mix32(adv, None, 2, 0, ma)
  assert abs(s.astype(F64).mean()) < 1e-6 and abs(s.astype(F64).std() - 1) < 1e-5


def test_lagrange_sequence_worked_by_hand():
  """lr 0.5, budget 2, lambda_max 3, every value a short binary fraction (exact in float32):
    start 1;  mean 3, 4 episodes -> 1 + 0.5 = 1.5;  mean 1 -> 1.0;  no episodes -> stays 1.0, count 0;
    mean -4 -> 1 - 3 = -2 -> 0;  mean 10 -> 0 + 4 -> 3 (the cap)."""
  s = np.array([1, 0, 0, 0], F32)
  steps = [([4, 3, 0, 0], [1.5, 3, 4, 1]), ([2, 1, 0, 0], [1.0, 1, 2, 2]), ([0, 99, 0, 0], [1.0, 1, 0, 2]),
           ([1, -4, 0, 0], [0.0, -4, 1, 3]), ([8, 10, 0, 0], [3.0, 10, 8, 4])]
  for mom, want in steps:
    s = R.lagrange32(s, np.array(mom, F32), 0.5, 2.0, 3.0)
    assert s.dtype == F32
    np.testing.assert_array_equal(s, np.array(want, F32))
  assert R.lagrange64(1.0, 3.0, 0.5, 2.0, 3.0) == 1.5 and R.lagrange64(1.0, -4.0, 0.5, 2.0) == 0.0
  assert R.lagrange32([1, 0, 0, 0], [1, 100, 0, 0], 0.5, 2.0)[0] == 50.0   # no cap by default


def test_clip_against_linalg_norm():
  g = np.random.RandomState(4).normal(size=6000).astype(F32)
  norm, factor = R.clip64(g, 0.5)
  np.testing.assert_allclose(norm, np.linalg.norm(g.astype(F64)), rtol=1e-14)
  assert factor == 0.5 / (norm + 1e-6)
  n32, f32, out = R.clip32(g, 0.5)
  assert abs(n32 - norm) / norm < 1e-5 and abs(f32 - factor) / factor < 1e-5
  np.testing.assert_array_equal(out, (g * f32).astype(F32))
  n32, f32, out = R.clip32(g, 1e6)
  assert f32 == 1 and out.tobytes() == g.tobytes()
  n32, f32, out = R.clip32(np.zeros(9, F32), 0.5)
  assert n32 == 0 and f32 == 1

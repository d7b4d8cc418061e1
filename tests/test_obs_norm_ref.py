"""tests/obs_norm_ref.py pinned without a GPU: the running moments against np.mean / np.var of the concatenation, the float32
restatement against the float64 one, the table's convention, and normalize32's clamp and NaN behaviour by hand-worked values."""
import numpy as np

import obs_norm_ref as O

F32, F64 = np.float32, np.float64


def _batches(od=12):
  rng = np.random.RandomState(5)
  scale = 10.0**rng.uniform(-3, 3, od)
  mean = rng.uniform(-2, 2, od) * scale
  return [(mean + scale * rng.normal(size=(n, od))).astype(F32) for n in (7, 33, 130)]


def test_merged_batches_equal_the_moments_of_the_concatenation():
  bs = _batches()
  state = O.empty_state(12)
  for b in bs:
    state = O.merge(state, O.batch_moments(b))
  x = np.concatenate(bs).astype(F64)
  assert state[0] == 170
  np.testing.assert_allclose(state[1:13], np.mean(x, axis=0), rtol=1e-12, atol=0)
  np.testing.assert_allclose(state[13:] / state[0], np.var(x, axis=0), rtol=1e-12, atol=0)
  # one batch into the empty state is that batch exactly
  one = O.batch_moments(bs[1])
  first = O.merge(O.empty_state(12), one)
  assert first[0] == 33 and (first[1:13] == one[1]).all() and (first[13:] == one[2]).all()


def test_float32_restatement_is_close_and_never_negative():
  for b in _batches():
    n, m64, q64 = O.batch_moments(b)
    n32, m32, q32 = O.batch_moments(b, F32)
    assert n32 == n and (q32 >= 0).all()
    std = np.sqrt(q64 / n)
    assert (np.abs(m32 - m64) <= 1e-5 * std).all()
    assert (np.abs(q32 - q64) <= 1e-5 * q64).all()
  # a constant column: the shifted second pass gives exactly 0
  c = np.full((130, 4), 1.5, F32)
  n, m, q = O.batch_moments(c, F32)
  assert (m == 1.5).all() and (q == 0).all()


def test_table_convention_and_identity():
  od = 3
  state = np.array([4.0, 1.0, -2.0, 0.5, 4.0 * 4.0, 0.0, 4.0 * 0.25], F64)   # var 4, 0, 0.25
  t = O.table32(state, 1e-8)
  assert t.dtype == F32 and t.shape == (2, od)
  np.testing.assert_array_equal(t[0], np.array([1.0, -2.0, 0.5], F32))
  eps = F64(F32(1e-8))
  np.testing.assert_array_equal(t[1], np.array([1 / np.sqrt(4 + eps), 1 / np.sqrt(eps), 1 / np.sqrt(0.25 + eps)]).astype(F32))
  assert t[1][0] == F32(0.5) and t[1][2] == F32(2.0)
  ident = O.table32(O.empty_state(od), 1e-8)
  np.testing.assert_array_equal(ident, np.array([[0, 0, 0], [1, 1, 1]], F32))
  assert O.measure(state, state) == dict(mean=0.0, M2=0.0)


def test_near_constant_columns_are_judged_apart():
  """Column 1 is the same value in every row of either batch; a float32 implementation carries its mean to 2^-24 and turns
  that into an M2 of rounding noise.  measure() skips it under resolved() and near_constant_ok() bounds it."""
  rng = np.random.RandomState(2)
  a = np.stack([rng.normal(1.0, 0.5, 40), np.full(40, 0.1), np.zeros(40)], 1).astype(F32)
  ref = O.merge(O.merge(O.empty_state(3), O.batch_moments(a[:15])), O.batch_moments(a[15:]))
  noisy = ref.copy()
  noisy[2] *= 1 + 2.0**-23           # the mean of column 1 off by two units in its last float32 place
  noisy[5] = 40 * (0.1 * 2.0**-24)**2   # and an M2 of that size where the reference has none
  assert list(O.resolved(ref)) == [True, True, True] and list(O.resolved(noisy)) == [True, False, True]
  assert O.near_constant_ok(noisy, noisy) and O.near_constant_ok(ref, noisy)
  off = noisy.copy()
  off[2] = 0.1001
  assert not O.near_constant_ok(off, noisy)
  assert O.measure(off, noisy, O.resolved(noisy)) == dict(mean=0.0, M2=0.0) and O.measure(off, noisy)['mean'] > 1


def test_normalize32_by_hand():
  table = np.array([[1.0, 0.0, -2.0, 0.5], [2.0, 100.0, 0.5, 4.0]], F32)
  x = np.array([[1.5, 0.25, 0.0, np.nan], [-9.0, -0.02, 40.0, 0.5], [np.inf, 0.049, -2.0, -np.inf]], F32)
  got = O.normalize32(x, table, 5.0)
  want = np.array([[1.0, 5.0, 1.0, np.nan], [-5.0, -2.0, 5.0, 0.0], [5.0, F32(F32(0.049) * F32(100.0)), 0.0, -5.0]], F32)
  np.testing.assert_array_equal(got, want)
  assert got.dtype == F32 and np.isnan(got[0, 3])
  # every operation is rounded on its own: fl(fl(x - m) * r), not a fused or float64 evaluation
  xs, m, r = F32(1.0000001), F32(0.3333333), F32(3.0000002)
  one = O.normalize32(np.array([[xs]], F32), np.array([[m], [r]], F32), np.inf)[0, 0]
  assert one == F32(F32(xs - m) * r)
  # clip = inf clamps nothing, and the identity table returns x bit for bit (x - 0 and * 1 are exact)
  ident = np.stack([np.zeros(4, F32), np.ones(4, F32)])
  big = np.array([[1e30, -1e30, 3.5, -0.0]], F32)
  np.testing.assert_array_equal(O.normalize32(big, ident, np.inf), big)

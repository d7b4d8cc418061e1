"""Pins tests/policy_grad_ref.py, the reference of test_policy_grad.py, without a GPU: the float64 gradient against central
differences of the float64 loss, the float32 Adam chain against a float64 Adam, and the clamp's edge cases."""
import numpy as np
import pytest

import policy_grad_ref as G
import policy_ref as P

F32 = np.float32
ROBOTS = {'point': (60, 2), 'car': (72, 2), 'doggo': (104, 12)}


@pytest.mark.parametrize('robot,hidden,rows,activation', [('point', 64, 130, 'relu'), ('doggo', 96, 65, 'relu'), ('car', 32, 33, 'tanh'),
                                                          ('doggo', 32, 40, 'tanh'), ('point', 32, 50, 'tanh'), ('car', 64, 70, 'relu')])
def test_float64_gradient_agrees_with_central_differences(robot, hidden, rows, activation):
  """h = 1e-6 on two random entries of every tensor: 1e-6 relative to the tensor's largest gradient entry.  A ReLU unit whose
  pre-activation crosses zero inside +-h would break the difference, not the gradient: with a few thousand pre-activations
  of order one and h = 1e-6 that does not happen in these seeded cases."""
  od, nu = ROBOTS[robot]
  rng = np.random.RandomState(7 * hidden + rows)
  prm = {k: v.astype(np.float64) for k, v in P.random_params(rng, od, nu, hidden).items()}
  batch = G.make_batch(rng, prm, rows, activation)
  coef = dict(G.COEF, scale=1.0 / rows)
  loss, grad, stats = G.loss_grad64(prm, batch, coef, None, activation)
  assert np.isfinite(loss) and stats[5] == pytest.approx(1.0) and 0 < stats[4] < 1
  h = 1e-6
  worst = 0.0
  for k in P.KEYS:
    for _ in range(2):
      idx = tuple(rng.randint(0, s) for s in prm[k].shape)
      side = []
      for sign in (+1, -1):
        q = {kk: v.copy() for kk, v in prm.items()}
        q[k][idx] += sign * h
        side.append(G.loss_grad64(q, batch, coef, None, activation)[0])
      fd = (side[0] - side[1]) / (2 * h)
      err = abs(fd - grad[k][idx]) / np.abs(grad[k]).max()
      worst = max(worst, err)
      assert err <= 1e-6, (k, idx, fd, grad[k][idx])
  print(f'{robot} {hidden} {rows} {activation}: worst relative difference {worst:.2e}')


def test_float32_restatement_is_close_and_absent_cost_terms_vanish():
  rng = np.random.RandomState(3)
  prm = P.random_params(rng, 60, 2, 64)
  batch = G.make_batch(rng, prm, 130)
  coef = dict(G.COEF, scale=1.0 / 130)
  masks = G.relu_masks(prm, batch['obs'])
  l64, g64, s64 = G.loss_grad64(prm, batch, coef, masks)
  l32, g32, s32 = G.loss_grad32(prm, batch, coef, masks)
  m = G.measure((g32, s32), (g64, s64))
  assert max(m.values()) < 2e-5 and abs(l32 - l64) < 1e-5 * abs(l64), m   # fp32: some 1e-7 per operation, sums of 130 rows
  assert g32['W1'].dtype == F32
  # without the cost arrays: no cost critic, statistic 2 zero, the advantage is the reward channel's
  b2 = dict(batch, cadv=None, cret=None)
  _, g, s = G.loss_grad64(prm, b2, coef, masks)
  _, gz, sz = G.loss_grad64(prm, batch, dict(coef, cadv_mul=0.0, cvf_coef=0.0), masks)
  assert s[2] == 0 and sz[2] > 0 and all(np.array_equal(g[k], gz[k]) for k in P.KEYS)
  assert (g['W3'][:, 3] == 0).all()
  flat = G.flat(g, s)
  back, st = G.split(flat, P.shapes(60, 2, 64))
  assert len(flat) == 8326 + 8 and np.array_equal(back['W2'], g['W2']) and np.array_equal(st, s)


def test_adam_chain_agrees_with_float64_and_clamps():
  rng = np.random.RandomState(5)
  n = 1000
  p, g = rng.standard_normal(n).astype(F32), (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(F32)
  m32, v32, p32 = np.zeros(n, F32), np.zeros(n, F32), p.copy()
  m64, v64, p64 = np.zeros(n), np.zeros(n), p.astype(np.float64)
  b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-3
  f1, f2 = float(F32(b1)), float(F32(b2))   # the moments use the float32 betas: 1 - fl(0.999) is 1.3e-5 off 0.001
  for t in (1, 2, 3, 4):
    step = G.adam_step_size(lr, t)
    p32, m32, v32 = G.adam_ref32(p32, g, m32, v32, step)
    m64 = f1 * m64 + (1 - f1) * g
    v64 = f2 * v64 + (1 - f2) * g.astype(np.float64) ** 2
    p64 = p64 - lr * np.sqrt(1 - b2**t) / (1 - b1**t) * m64 / (np.sqrt(v64) + eps)
    assert p32.dtype == F32 and np.abs(p32 - p64).max() <= 1e-6 * max(1.0, np.abs(p64).max())
  assert np.abs(m32 - m64).max() <= 1e-6 * np.abs(m64).max() and np.abs(v32 - v64).max() <= 1e-6 * np.abs(v64).max()
  # the clamp: from clamp_first on, nothing before it; clamp_first == n clamps nothing, 0 everything
  p0 = np.array([-1.0, 0.2, -3.0, 0.04, 5.0], F32)
  z = np.zeros(5, F32)
  for first, want in ((5, p0), (0, np.maximum(p0, F32(0.05))), (3, np.array([-1.0, 0.2, -3.0, 0.05, 5.0], F32))):
    got, m, v = G.adam_ref32(p0, z, z, z, 1e-3, clamp_first=first, clamp_lo=0.05)
    np.testing.assert_array_equal(got, want)
    assert not m.any() and not v.any()   # a zero gradient moves nothing: 0 / (0 + eps)
  got, _, _ = G.adam_ref32(p0, z, z, z, 1e-3)   # the default clamps nothing
  np.testing.assert_array_equal(got, p0)
  # a denormal gradient: v underflows to zero, m stays a denormal, the step is finite
  got, m, v = G.adam_ref32(np.ones(1, F32), np.full(1, 1e-41, F32), np.zeros(1, F32), np.zeros(1, F32), 1e-3)
  assert np.isfinite(got).all() and v[0] == 0 and 0 < m[0] < np.finfo(F32).tiny

"""The actor-critic forward on the device (csrc/sag_policy.hpp, sag_policy_forward_device, sag.MLPPolicy) against the NumPy
restatement of tests/policy_ref.py - an exact fmaf chain in the header's order, checked against libm in test_policy_ref.py -
never against the kernel's own arithmetic.  The ReLU network is compared bit for bit; what rests on hardware transcendentals
(tanh, the normals) is compared with float64 under four times the largest error measured once on the MI355X - and tanh, for
every built hidden size, under eight times the error of the restatement's own float32 evaluation of that case.  The forward,
sampling and refusal cases at <= 130 rows and hidden <= 96 also run on the host build of the device sources
(test_policy_hostemu.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import policy_ref as P
import rollout_ref as R
from test_device_reset import KEY

F32 = np.float32
HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
ERR_ARG = -1      # SAG_ERR_ARG
MEAN = 1          # SAG_POLICY_MEAN
SENTINEL = 7.0    # what output rows at or beyond n_rows hold before and after a call
GUARD = 3         # such rows behind every output
ROBOTS = {'point': (60, 2), 'car': (72, 2), 'doggo': (104, 12)}
# measured maxima on the MI355X (docstrings of the tests that assert them), asserted with the factor 4
TANH_MEASURED = 5.648e-7
ACTION_MEASURED = 4.212e-7
LOGP_MEASURED = 3.734e-6


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctxs(nat):
  made = {}

  def get(robot):
    if robot not in made:
      made[robot] = nat.Context(robot, 8, seed=KEY)   # n_rows is not n_envs
    return made[robot]
  yield get
  for c in made.values():
    c.close()


class _Call:
  """One sag_policy_forward_device call on fresh buffers: obs [rows, pitch] uploaded as given (pad columns included), every
  output allocated for rows + GUARD rows and filled with SENTINEL."""

  def __init__(self, nat, c, prm, obs, hidden, pitch=None, activation=0, flags=0, draw=0, row0=0, n_rows=None, logp_const=0.25,
               outputs=('actions', 'logp', 'value', 'cvalue')):
    self.nat, self.c = nat, c
    od, nu = c.info['obs_dim'], c.info['nu']
    rows = len(obs)
    self.rows, self.nu = rows, nu
    self.shape = {'actions': (rows + GUARD, nu), 'logp': (rows + GUARD,), 'value': (rows + GUARD,), 'cvalue': (rows + GUARD,)}
    self.p = {'params': c.dev_alloc(len(prm) * 4 + 16), 'obs': c.dev_alloc(obs.nbytes + 16)}
    c.dev_upload(self.p['params'], np.ascontiguousarray(prm, F32))
    c.dev_upload(self.p['obs'], np.ascontiguousarray(obs, F32))
    for k in outputs:
      self.p[k] = c.dev_alloc(int(np.prod(self.shape[k])) * 4)
      c.dev_upload(self.p[k], np.full(self.shape[k], SENTINEL, F32))
    out = [self.p[k].value if k in outputs else None for k in ('actions', 'logp', 'value', 'cvalue')]
    self.desc = nat.PolicyDesc(rows if n_rows is None else n_rows, hidden, activation, flags, obs.shape[1] if pitch is None else pitch, 0,
                               draw & 0xffffffff, row0 & 0xffffffff, logp_const, self.p['params'].value, self.p['obs'].value, *out)

  def run(self):
    rc = self.c.lib.sag_policy_forward_device(self.c.h, C.byref(self.desc))
    self.c.wait()
    return rc

  def get(self, k):
    return self.c.dev_download(self.p[k], self.shape[k], F32)

  def untouched(self, from_row=None):
    """Every output row at or beyond from_row (default: n_rows) still holds the sentinel."""
    r0 = self.desc.n_rows if from_row is None else from_row
    return all((self.get(k)[r0:] == F32(SENTINEL)).all() for k in self.shape if k in self.p)

  def free(self):
    for p in self.p.values():
      self.c.dev_free(p)
    self.p = {}


def _obs(rng, rows, od, pad=0):
  obs = np.full((rows, od + pad), np.nan, F32)   # NaN in the pad columns: a read of one poisons its row
  obs[:, :od] = rng.uniform(-1.5, 1.5, (rows, od))
  return obs


def _check_bits(nat, c, prm, obs, hidden, n_rows=None, what=''):
  """ReLU with SAG_POLICY_MEAN: actions (= the mean), value and cost value equal forward_ref32 bit for bit, logp = -S, and
  nothing at or beyond n_rows is written."""
  od, nu = c.info['obs_dim'], c.info['nu']
  n = len(obs) if n_rows is None else n_rows
  k = _Call(nat, c, P.pack(prm), obs, hidden, flags=MEAN, n_rows=n, logp_const=0.25)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  mean, v, cv = P.forward_ref32(prm, obs[:n, :od])
  assert np.isfinite(mean).all() and np.isfinite(v).all()
  np.testing.assert_array_equal(k.get('actions')[:n], mean, err_msg=f'{what}: mean')
  np.testing.assert_array_equal(k.get('value')[:n], v, err_msg=f'{what}: value')
  np.testing.assert_array_equal(k.get('cvalue')[:n], cv, err_msg=f'{what}: cost value')
  np.testing.assert_array_equal(k.get('logp')[:n], np.full(n, -0.25, F32), err_msg=f'{what}: logp')
  assert k.untouched(), f'{what}: a write at or beyond n_rows'
  k.free()
  return mean, v, cv


# every value of each axis at least once; hidden 256 at 65 rows only (and not on the host build)
FORWARD_CASES = [('point', 32, 1), ('point', 64, 31), ('car', 96, 32), ('car', 32, 33), ('doggo', 64, 64), ('point', 96, 65),
                 ('doggo', 96, 130), ('car', 64, 130)] + ([] if HOSTEMU else [('doggo', 256, 65), ('point', 256, 65)])
# every built instance (NT = hidden / 32 = 1 ... 8: the weight ring is D = 16, 8, 5, 4, 3, 2, 2, 2 k-steps deep) under every
# robot (layer 1 has 30, 36 or 52 k-steps, so whether its last ring pass is partial depends on both) at 33 rows: one full
# tile and a tile of one row.  car/32/33 is in the list above.
HIDDENS = tuple(range(32, 257, 32))
FORWARD_MATRIX = [(robot, hidden, 33) for hidden in HIDDENS for robot in ('point', 'car', 'doggo')
                  if (robot, hidden, 33) not in FORWARD_CASES and not (HOSTEMU and hidden >= 128)]


@pytest.mark.gpu
@pytest.mark.parametrize('robot,hidden,rows', FORWARD_CASES + FORWARD_MATRIX)
def test_forward_relu_equals_the_fmaf_chains_bit_for_bit(nat, ctxs, robot, hidden, rows):
  c = ctxs(robot)
  od, nu = ROBOTS[robot]
  rng = np.random.RandomState(1000 * hidden + rows)
  prm = P.random_params(rng, od, nu, hidden, scale=1.5)
  _check_bits(nat, c, prm, _obs(rng, rows, od), hidden, what=f'{robot} {hidden} {rows}')


@pytest.mark.gpu
def test_forward_reads_a_pitched_observation_array_and_no_pad_column(nat, ctxs):
  """obs_pitch = obs_dim + 4 with NaN in the four pad columns, 33 of 40 uploaded rows asked for: rows at or beyond n_rows are
  neither read (they are NaN throughout) nor written."""
  for robot, hidden in (('point', 64), ('doggo', 32)):
    c = ctxs(robot)
    od, nu = ROBOTS[robot]
    rng = np.random.RandomState(77)
    obs = _obs(rng, 40, od, pad=4)
    obs[33:] = np.nan
    _check_bits(nat, c, P.random_params(rng, od, nu, hidden), obs, hidden, n_rows=33, what=f'{robot} pitched')


@pytest.mark.gpu
@pytest.mark.parametrize('robot,H', [('car', 96)] + ([] if HOSTEMU else [('car', 128), ('doggo', 160)]))
def test_forward_directed_weights(nat, ctxs, robot, H):
  """W1 a rectangular identity with W2 and W3 asymmetric (a transposed or row-swapped tile cannot pass: the guide's A = I check
  with asymmetric B), every bias zero, and every weight zero - which returns the biases.  Car at hidden 96 and 128 (ring depths
  5 and 4), Doggo at 160 (depth 3, where the 52 k-steps of layer 1 end in a ring pass of one)."""
  c = ctxs(robot)
  od, nu = ROBOTS[robot]
  rows = 65
  rng = np.random.RandomState(3)
  obs = _obs(rng, rows, od)
  obs[:, :od] = np.abs(obs[:, :od])                # the identity layer then passes its inputs through the relu unchanged
  prm = P.random_params(rng, od, nu, H)
  prm['W1'] = np.eye(od, H, dtype=F32)
  prm['b1'][:] = 0
  j, k = np.meshgrid(np.arange(H), np.arange(H))   # W2[k][j] = (3 k + 7 j + 1) / 1024: exact in fp32, W2 != W2^T
  prm['W2'] = ((3 * k + 7 * j + 1) / 1024.0).astype(F32)
  prm['W3'] = ((np.arange(H)[:, None] * 5 + np.arange(nu + 2)[None, :] * 11 + 1) / 4096.0).astype(F32)
  assert not np.array_equal(prm['W2'], prm['W2'].T)
  mean, v, cv = _check_bits(nat, c, prm, obs, H, what='identity')
  h1 = np.zeros((rows, H), F32)
  h1[:, :od] = obs[:, :od]
  h2 = np.maximum(h1.astype(np.float64) @ prm['W2'].astype(np.float64) + prm['b2'], 0)
  o = h2 @ prm['W3'].astype(np.float64) + prm['b3']
  # and the reference is the network: two layers of K = H all-positive products, (K + 2) 2^-24 each
  assert np.abs(np.concatenate([mean, v[:, None], cv[:, None]], 1) - o).max() <= 2 * (H + 2) * 2.0**-24 * np.abs(o).max()
  zb = P.random_params(rng, od, nu, H)
  for b in ('b1', 'b2', 'b3'):
    zb[b][:] = 0
  _check_bits(nat, c, zb, obs, H, what='zero biases')
  zw = P.random_params(rng, od, nu, H)
  for w in ('W1', 'W2', 'W3'):
    zw[w][:] = 0
  zw['b3'] = np.arange(1, nu + 3, dtype=F32)
  mean, v, cv = _check_bits(nat, c, zw, obs, H, what='zero weights')
  assert (mean == zw['b3'][:nu]).all() and (v == zw['b3'][nu]).all() and (cv == zw['b3'][nu + 1]).all()


@pytest.mark.gpu
def test_forward_tanh_against_float64(nat, ctxs):
  """tanh, hidden 64, 130 rows: the largest |output - forward_ref64| measured on the MI355X is 5.648e-7 (outputs up to 1.43);
  asserted with the factor 4.  The form 1 - 2 / (exp2(c x) + 1) loses relative accuracy near 0, not absolute."""
  c = ctxs('point')
  od, nu = ROBOTS['point']
  rng = np.random.RandomState(21)
  prm = P.random_params(rng, od, nu, 64, scale=1.5)
  obs = _obs(rng, 130, od)
  k = _Call(nat, c, P.pack(prm), obs, 64, activation=1, flags=MEAN)
  assert k.run() == 0
  m64, v64, c64 = P.forward_ref64(prm, obs, 'tanh')
  err = max(np.abs(k.get('actions')[:130] - m64).max(), np.abs(k.get('value')[:130] - v64).max(), np.abs(k.get('cvalue')[:130] - c64).max())
  print(f'tanh: max |output - float64| = {err:.3e}, max |output| = {max(np.abs(m64).max(), np.abs(v64).max(), np.abs(c64).max()):.3f}')
  assert k.untouched()
  assert err <= 4 * TANH_MEASURED
  k.free()


TANH_FACTOR = 8.0   # test_policy_grad.py's: the same terms as the float32 restatement, exp2 and rcp of the 1 ulp class
# one case per built instance, the robots in rotation (each at least twice, doggo/160 among them)
TANH_CASES = [('point', 32), ('car', 64), ('doggo', 96)] + (
    [] if HOSTEMU else [('point', 128), ('doggo', 160), ('car', 192), ('point', 224), ('doggo', 256)])


@pytest.mark.gpu
@pytest.mark.parametrize('robot,hidden', TANH_CASES)
def test_forward_tanh_of_every_instance_against_float64(nat, ctxs, robot, hidden):
  """tanh at 33 rows for every hidden size.  The tolerance is per case: the error of the reference's own float32 restatement,
  max |forward_ref32(tanh) - forward_ref64| over the three outputs, times 8 - the device sums the same terms in the same order
  and differs in the hardware exp2 and reciprocal only, while an indexing fault moves an output by the order of the output.
  Measured on the MI355X, max |device - float64| beside the float32 restatement's own error (DESIGN.md 3.8 has the table):
  point/32 2.71e-7 / 2.35e-7, car/64 2.95e-7 / 3.87e-7, doggo/96 5.02e-7 / 4.42e-7, point/128 4.12e-7 / 6.47e-7, doggo/160
  8.44e-7 / 7.93e-7, car/192 8.00e-7 / 7.51e-7, point/224 8.22e-7 / 7.63e-7, doggo/256 5.77e-7 / 5.89e-7: at most 1.16 times it."""
  c = ctxs(robot)
  od, nu = ROBOTS[robot]
  rows = 33
  rng = np.random.RandomState(7000 + hidden)
  prm = P.random_params(rng, od, nu, hidden, scale=1.5)
  obs = _obs(rng, rows, od)
  k = _Call(nat, c, P.pack(prm), obs, hidden, activation=1, flags=MEAN)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  r64 = P.forward_ref64(prm, obs, 'tanh')
  r32 = P.forward_ref32(prm, obs, 'tanh')
  got = k.get('actions')[:rows], k.get('value')[:rows], k.get('cvalue')[:rows]
  own = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, r64))
  err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, r64))
  top = max(float(np.abs(b).max()) for b in r64)
  print(f'tanh {robot} {hidden}: max |device - float64| = {err:.3e}, max |float32 restatement - float64| = {own:.3e}, '
        f'tolerance {TANH_FACTOR * own:.3e}, max |output| = {top:.3f}')
  assert k.untouched()
  assert own > 0 and np.isfinite(err)
  assert err <= TANH_FACTOR * own
  k.free()


@pytest.mark.gpu
def test_sampling_against_float64_and_across_draws_keys_and_rows(nat, ctxs):
  """Actions and logp against float64 formed from the device's OWN mean (downloaded with SAG_POLICY_MEAN) and normals_ref:
  measured on the MI355X, max |action - float64| = 4.212e-7 (Doggo: |z| up to 3.58, std up to 1.2; Point 1.649e-7) and
  max |logp - float64| = 3.734e-6 (Doggo: |logp| up to 21.7; Point 4.838e-7); both asserted with the factor 4, which covers the
  hardware log2, sin and cos.  The same draw repeats its bits; another draw, key or row0 changes more than 90 % of the elements;
  SAG_POLICY_MEAN gives the mean and logp = -S.  Doggo at hidden 128 and 256, 33 rows (its 12 actions take all three Philox
  blocks and both halves of z), under the same bounds: measured 2.92e-7 / 1.57e-6 and 2.90e-7 / 1.57e-6 (|logp| up to 19.4)."""
  for robot, hidden, rows in (('doggo', 32, 130), ('point', 64, 65)) + (() if HOSTEMU else (('doggo', 128, 33), ('doggo', 256, 33))):
    c = ctxs(robot)
    od, nu = ROBOTS[robot]
    rng = np.random.RandomState(9)
    prm = P.random_params(rng, od, nu, hidden)
    S = P.logp_const(prm['std'])
    obs = _obs(rng, rows, od)
    kw = dict(logp_const=S)

    def sample(**over):
      k = _Call(nat, c, P.pack(prm), obs, hidden, **dict(kw, **over))
      assert k.run() == 0
      assert k.untouched()
      out = k.get('actions')[:rows], k.get('logp')[:rows], k.get('value')[:rows], k.get('cvalue')[:rows]
      k.free()
      return out

    mean, lp0, v, cv = sample(flags=MEAN, draw=5)
    np.testing.assert_array_equal(lp0, np.full(rows, -F32(S), F32), err_msg='logp of the mean is -S')
    ref = P.forward_ref32(prm, obs)
    np.testing.assert_array_equal(mean, ref[0])
    a, lp, v2, cv2 = sample(draw=5)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(cv2, cv)
    z = P.normals_ref(KEY, 0, rows, 5, nu)
    want = mean.astype(np.float64) + prm['std'].astype(np.float64)[None, :] * z
    want_lp = -0.5 * (z * z).sum(axis=1) - S
    ea, el = float(np.abs(a - want).max()), float(np.abs(lp - want_lp).max())
    print(f'{robot} {hidden}: max |action - float64| = {ea:.3e} (max |z| {np.abs(z).max():.2f}), max |logp - float64| = {el:.3e} '
          f'(max |logp| {np.abs(want_lp).max():.1f})')
    assert ea <= 4 * ACTION_MEASURED and el <= 4 * LOGP_MEASURED
    b = sample(draw=5)
    np.testing.assert_array_equal(b[0], a, err_msg='the same draw')
    np.testing.assert_array_equal(b[1], lp)
    assert (sample(draw=6)[0] != a).mean() > 0.9, 'another draw'
    shifted = sample(draw=5, row0=1)[0]
    assert (shifted != a).mean() > 0.9, 'another row0'
    zs = P.normals_ref(KEY, 1, rows, 5, nu)
    assert np.abs(shifted - (mean.astype(np.float64) + prm['std'].astype(np.float64)[None, :] * zs)).max() <= 4 * ACTION_MEASURED
    c.set_seed(KEY ^ (1 << 40))
    assert (sample(draw=5)[0] != a).mean() > 0.9, 'another key'
    c.set_seed(KEY)
    # without d_actions nothing is sampled: the value-only evaluation
    k = _Call(nat, c, P.pack(prm), obs, hidden, draw=5, outputs=('logp', 'value', 'cvalue'), **kw)
    assert k.run() == 0
    np.testing.assert_array_equal(k.get('logp')[:rows], lp0)
    np.testing.assert_array_equal(k.get('value')[:rows], v)
    k.free()


@pytest.mark.gpu
def test_sampling_statistics(nat, ctxs):
  """(a - mean) / std over 1700 Doggo rows x 12 = 20 400 values: mean and variance within 4 standard errors of 0 and 1, the
  bounds of test_throughput_rng.py."""
  c = ctxs('doggo')
  od, nu = ROBOTS['doggo']
  rows = 1700
  rng = np.random.RandomState(2)
  prm = P.random_params(rng, od, nu, 32)
  obs = _obs(rng, rows, od)
  out = []
  for flags in (MEAN, 0):
    k = _Call(nat, c, P.pack(prm), obs, 32, flags=flags, draw=123456)
    assert k.run() == 0
    out.append(k.get('actions')[:rows].astype(np.float64))
    k.free()
  x = ((out[1] - out[0]) / prm['std'].astype(np.float64)[None, :]).ravel()
  n = len(x)
  assert n >= 20000 and np.isfinite(x).all()
  assert abs(x.mean()) < 4 / math.sqrt(n), x.mean()
  assert abs(x.var() - 1) < 4 * math.sqrt(2 / (n - 1)), x.var()


@pytest.mark.gpu
def test_refusals_enqueue_nothing_and_null_outputs_are_honoured(nat, ctxs):
  c = ctxs('point')
  od, nu = ROBOTS['point']
  rng = np.random.RandomState(4)
  prm = P.random_params(rng, od, nu, 32)
  obs = _obs(rng, 33, od)
  bad = [('hidden', 0), ('hidden', 16), ('hidden', 48), ('hidden', 288), ('hidden', -32), ('activation', 2), ('activation', -1),
         ('flags', 2), ('flags', -1), ('obs_pitch', od - 4), ('obs_pitch', od + 2), ('n_rows', 0), ('n_rows', -5),
         ('logp_const', float('nan')), ('logp_const', float('inf')), ('d_params', None), ('d_obs', None)]
  bad += [(f, 'misaligned') for f in ('d_params', 'd_obs', 'd_actions', 'd_logp', 'd_value', 'd_cvalue')]
  for field, v in bad:
    k = _Call(nat, c, P.pack(prm), obs, 32)
    if v == 'misaligned':
      v = getattr(k.desc, field) + (8 if field == 'd_obs' else 2)   # d_obs: 8-byte aligned is not enough
    setattr(k.desc, field, v)
    assert k.run() == ERR_ARG, (field, v)
    assert c.lib.sag_last_error(c.h).decode().startswith('sag_policy_forward_device:')
    assert k.untouched(0), f'{field} = {v}: refused, but an output was written'
    k.free()
  assert c.lib.sag_policy_forward_device(c.h, None) == ERR_ARG
  assert c.lib.sag_policy_forward_device(None, None) == ERR_ARG
  # the context is usable after the refusals, and every output may be left out on its own
  full = _Call(nat, c, P.pack(prm), obs, 32, draw=3)
  assert full.run() == 0
  names = ('actions', 'logp', 'value', 'cvalue')
  for drop in names:
    k = _Call(nat, c, P.pack(prm), obs, 32, draw=3, outputs=tuple(n for n in names if n != drop))
    assert k.run() == 0
    for n in names:
      if n == drop:
        continue
      if drop == 'actions' and n == 'logp':   # nothing is sampled without d_actions
        np.testing.assert_array_equal(k.get(n)[:33], np.full(33, -0.25, F32))
      else:
        np.testing.assert_array_equal(k.get(n), full.get(n), err_msg=f'{n} without {drop}')
    k.free()
  k = _Call(nat, c, P.pack(prm), obs, 32, outputs=())   # nothing to write: legal
  assert k.run() == 0
  k.free(); full.free()


# ----------------------------------------------------------------------------------------------------------------------
# sag.MLPPolicy with sag.RolloutBuffer
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_policy_closes_the_rollout_loop_on_the_device(nat):
  """Point, 130 envs, T = 5, time limit 3, hidden 32, a deterministic policy: collect, evaluate and advantages on device views
  only; then forward_ref32 of the downloaded observations reproduces actions, values and final values, and gae_ref32 of the
  downloaded arrays the advantages and returns of both channels, all bit for bit."""
  import safe_adaptation_gym_amd as sag
  from test_reset_loop import _make_env
  n, T = 130, 5
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=3, device_buffers=True, time_limit=3, auto_reset=True)
  env.reset()
  pi = sag.MLPPolicy(env, hidden=32, seed=1)
  pi.deterministic = True
  prm = pi.get_params()
  assert set(prm) == set(P.KEYS) and all(prm[k].shape == P.shapes(60, 2, 32)[k] for k in prm)
  assert all(np.abs(prm[k]).max() <= 1 / math.sqrt(s) for k, s in (('W1', 60), ('b1', 60), ('W2', 32), ('b2', 32), ('W3', 32), ('b3', 32)))
  np.testing.assert_array_equal(prm['std'], np.full(2, np.exp(-0.5), F32))
  np.testing.assert_array_equal(pi.params['W2'].numpy(), prm['W2'])
  assert pi.logp_const == P.logp_const(prm['std'])
  buf = sag.RolloutBuffer(env, steps=T)
  buf.collect(pi)
  pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  assert pi.draw == 0   # nothing was sampled
  obs, act, value, cvalue, logp = buf.obs.numpy(), buf.actions.numpy(), buf.value.numpy(), buf.cost_value.numpy(), buf.logp.numpy()
  for t in range(T + 1):
    mean, v, cv = P.forward_ref32(prm, obs[t])
    np.testing.assert_array_equal(value[t], v, err_msg=f'value[{t}]')
    np.testing.assert_array_equal(cvalue[t], cv, err_msg=f'cost_value[{t}]')
    if t < T:
      np.testing.assert_array_equal(act[t], mean, err_msg=f'actions[{t}]')
      np.testing.assert_array_equal(logp[t], np.full(n, -F32(pi.logp_const), F32))
  rows, count = buf.final_observations()
  done, slot = buf.done.numpy(), buf.final_slot.numpy()
  assert count == int((done != 0).sum()) >= n and (done == 2).any()   # the time limit of 3 truncates inside T = 5
  fv, fcv = buf.final_value.numpy(), buf.final_cost_value.numpy()
  _, v, cv = P.forward_ref32(prm, rows.numpy())
  np.testing.assert_array_equal(fv[:count], v)
  np.testing.assert_array_equal(fcv[:count], cv)
  reward, cost = buf.reward.numpy(), buf.cost.numpy()
  cap = buf.final_capacity
  adv, ret = R.gae_ref32_batch(reward, cost, done, value, 0.99, 0.95, slot, fv, cap)
  cadv, cret = R.gae_ref32_batch(reward, cost, done, cvalue, 0.99, 0.95, slot, fcv, cap, is_cost=True)
  for k, want in (('adv', adv), ('ret', ret), ('cadv', cadv), ('cret', cret)):
    np.testing.assert_array_equal(out[k].numpy(), want, err_msg=k)
  # a sampling policy advances its draw once per step and fills logp
  pi.deterministic = False
  buf.collect(pi)
  buf.wait()
  assert pi.draw == T
  a2, lp2, o2 = buf.actions.numpy(), buf.logp.numpy(), buf.obs.numpy()
  for t in (0, T - 1):
    mean, _, _ = P.forward_ref32(prm, o2[t])
    z = P.normals_ref(env._base_seed, 0, n, t, 2)
    assert np.abs(a2[t] - (mean.astype(np.float64) + float(prm['std'][0]) * z)).max() <= 4 * ACTION_MEASURED
    assert np.abs(lp2[t] - (-0.5 * (z * z).sum(axis=1) - pi.logp_const)).max() <= 4 * LOGP_MEASURED
  # a plain callable without act_into is asked as before
  calls = []

  def zeros(o, a):
    calls.append((o.shape, a.shape))
    a.ctx.dev_upload(nat.C.c_void_p(a.ptr), np.zeros(a.shape, F32))
  buf.collect(zeros)
  buf.wait()
  assert calls == [((n, 60), (n, 2))] * T and (buf.actions.numpy() == 0).all()
  # set_params round trip, and what the constructor refuses
  prm['std'] = np.array([0.5, 2.0], F32)
  pi.set_params(prm)
  assert pi.logp_const == P.logp_const(prm['std'])
  np.testing.assert_array_equal(pi.get_params()['std'], prm['std'])
  for kw in (dict(hidden=48), dict(hidden=512), dict(activation='gelu')):
    with pytest.raises(ValueError):
      sag.MLPPolicy(env, **kw)
  with pytest.raises(ValueError):
    sag.MLPPolicy(object())
  pi.close(); buf.close()

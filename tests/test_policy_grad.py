"""The PPO-Lagrangian update on the device (csrc/sag_policy_grad.hpp: sag_policy_backward_device, sag_adam_device,
MLPPolicy.backward, sag.PPOLearner) against the NumPy restatement of tests/policy_grad_ref.py, which test_policy_grad_ref.py
pins with central differences - never against the kernel's own arithmetic.

The gradient's tolerance is not a constant.  Per case the error of the reference's own float32 restatement (loss_grad32
against loss_grad64, max |a - b| / max |b| per tensor, the largest over the 7 tensors and the statistics) is computed, and the
device is granted 8 times that: it sums the same fp32 terms in another order and uses 1 ulp-class exp2 / log2 / rcp, while any
indexing fault costs at least one row's share, >= 1 / n ~ 2.5e-3 of a tensor's largest entry.  Adam is elementwise and compared
bit for bit.  The gradient, directed, Adam and refusal cases at <= 130 rows and hidden <= 96 also run on the host build of the
device sources (test_policy_grad_hostemu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import policy_grad_ref as G
import policy_ref as P
from test_device_reset import KEY

F32 = np.float32
HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
ERR_ARG, ERR_UNSUPPORTED = -1, -5
ACCUMULATE = 1
GUARD = 16          # words behind d_grad
SENTINEL = 7.0
FACTOR = 8.0
ROBOTS = {'point': (60, 2), 'car': (72, 2), 'doggo': (104, 12)}
INPUTS = ('obs', 'actions', 'logp_old', 'adv', 'ret', 'cadv', 'cret')


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
      made[robot] = nat.Context(robot, 8, seed=KEY)   # the rows of a batch are not n_envs
    return made[robot]
  yield get
  for c in made.values():
    c.close()


def _planes(a, n_rows, n_planes, pitch, pad_cols=0):
  """[n_planes * n_rows, ...] -> [n_planes, pitch, ... + pad_cols] with NaN in every pad row and pad column."""
  a = np.asarray(a, F32)
  tail = a.shape[1:]
  if pad_cols:
    tail = (tail[0] + pad_cols,)
  out = np.full((n_planes, pitch) + tail, np.nan, F32)
  src = a.reshape((n_planes, n_rows) + a.shape[1:])
  if pad_cols:
    out[:, :n_rows, :a.shape[1]] = src
  else:
    out[:, :n_rows] = src
  return out


class _Call:
  """One sag_policy_backward_device call: the batch of policy_grad_ref.make_batch laid out as n_planes planes of `pitch` rows
  (n_rows rounded up to 64) with NaN pad rows, d_grad of n_params + 8 + GUARD words filled with SENTINEL."""

  def __init__(self, nat, c, prm, batch, hidden, n_rows, n_planes, coef, activation='relu', flags=0, max_blocks=0, obs_pad=0,
               drop=()):
    self.nat, self.c = nat, c
    self.pitch = pitch = -(-n_rows // 64) * 64
    self.n_words = len(prm) + 8
    self.host = {k: _planes(batch[k], n_rows, n_planes, pitch, obs_pad if k == 'obs' else 0) for k in INPUTS}
    self.p = {k: c.dev_alloc(v.nbytes) for k, v in self.host.items()}
    for k, v in self.host.items():
      c.dev_upload(self.p[k], v)
    self.p['params'] = c.dev_alloc(len(prm) * 4)
    c.dev_upload(self.p['params'], np.ascontiguousarray(prm, F32))
    self.p['grad'] = c.dev_alloc((self.n_words + GUARD) * 4)
    self.fill(SENTINEL)
    ptr = lambda k: None if k in drop else self.p[k].value   # noqa: E731
    self.desc = nat.PolicyGradDesc(n_rows, n_planes, pitch, c.info['obs_dim'] + obs_pad, hidden, 0 if activation == 'relu' else 1, flags,
                                   max_blocks, coef['clip'], coef['vf_coef'], coef['cvf_coef'], coef['ent_coef'], coef['adv_mul'],
                                   coef['adv_sub'], coef['cadv_mul'], coef['cadv_sub'], coef['scale'], 0.0, ptr('params'), ptr('obs'),
                                   ptr('actions'), ptr('logp_old'), ptr('adv'), ptr('ret'), ptr('cadv'), ptr('cret'), ptr('grad'))

  def fill(self, value):
    self.c.dev_upload(self.p['grad'], np.full(self.n_words + GUARD, value, F32))

  def run(self):
    rc = self.c.lib.sag_policy_backward_device(self.c.h, C.byref(self.desc))
    self.c.wait()
    return rc

  def words(self):
    return self.c.dev_download(self.p['grad'], (self.n_words + GUARD,), F32)

  def grad(self):
    w = self.words()
    assert (w[self.n_words:] == F32(SENTINEL)).all(), 'a write behind d_grad'
    return w[:self.n_words]

  def inputs_unchanged(self):
    return all(self.c.dev_download(self.p[k], v.shape, F32).tobytes() == v.tobytes() for k, v in self.host.items())

  def free(self):
    for p in self.p.values():
      self.c.dev_free(p)
    self.p = {}


def _reference(prm, batch, coef, activation):
  """-> (float64 reference, tolerance): FACTOR times the largest measure of the float32 restatement."""
  masks = G.relu_masks(prm, batch['obs']) if activation == 'relu' else None
  _, g64, s64 = G.loss_grad64(prm, batch, coef, masks, activation)
  _, g32, s32 = G.loss_grad32(prm, batch, coef, masks, activation)
  own = G.measure((g32, s32), (g64, s64))
  assert all(np.isfinite(v) for v in own.values()), own
  return (g64, s64), FACTOR * max(own.values()), own


def _check(words, shapes, ref, tol, what):
  got = G.split(words.astype(np.float64), shapes)
  m = G.measure(got, ref)
  print(f'{what}: tolerance {tol:.3e}, device ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
  bad = {k: v for k, v in m.items() if not v <= tol}
  assert not bad, f'{what}: {bad} beyond {tol:.3e}'
  return m


def _setup(robot, hidden, rows, activation, seed=None):
  od, nu = ROBOTS[robot]
  rng = np.random.RandomState(1000 * hidden + rows if seed is None else seed)
  prm = P.random_params(rng, od, nu, hidden)
  batch = G.make_batch(rng, prm, rows, activation)
  return prm, batch, P.shapes(od, nu, hidden)


# (robot, hidden, n_rows, n_planes, activation): every value of each axis at least once; hidden 128 not on the host build
GRAD_CASES = [('point', 32, 1, 1, 'relu'), ('point', 64, 31, 3, 'relu'), ('car', 96, 32, 1, 'relu'), ('car', 32, 33, 3, 'tanh'),
              ('doggo', 64, 65, 1, 'relu'), ('doggo', 96, 130, 1, 'tanh'), ('doggo', 32, 33, 1, 'relu')] + (
                  [] if HOSTEMU else [('point', 128, 130, 1, 'relu'), ('doggo', 128, 33, 3, 'tanh'), ('car', 128, 65, 1, 'relu')])


@pytest.mark.gpu
@pytest.mark.parametrize('robot,hidden,rows,planes,activation', GRAD_CASES)
def test_gradient_and_statistics_against_the_float64_reference(nat, ctxs, robot, hidden, rows, planes, activation):
  """Measured on the MI355X (the figures are printed; DESIGN.md 3.9 has the table): the device stays below the float32
  restatement's own error in most tensors and below 8 times it in all."""
  c = ctxs(robot)
  prm, batch, shapes = _setup(robot, hidden, rows * planes, activation)
  coef = dict(G.COEF, scale=1.0 / (rows * planes))
  ref, tol, _ = _reference(prm, batch, coef, activation)
  k = _Call(nat, c, P.pack(prm), batch, hidden, rows, planes, coef, activation)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  _check(k.grad(), shapes, ref, tol, f'{robot} {hidden} {rows}x{planes} {activation}')
  assert k.inputs_unchanged()
  k.free()


@pytest.mark.gpu
def test_gradient_reads_pitched_observations_and_no_pad_column(nat, ctxs):
  """obs_pitch = obs_dim + 4 with NaN in the pad columns (and, as everywhere, in the pad rows of every plane)."""
  c = ctxs('point')
  prm, batch, shapes = _setup('point', 64, 33 * 3, 'relu', seed=5)
  coef = dict(G.COEF, scale=1.0 / 99)
  ref, tol, _ = _reference(prm, batch, coef, 'relu')
  k = _Call(nat, c, P.pack(prm), batch, 64, 33, 3, coef, obs_pad=4)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  _check(k.grad(), shapes, ref, tol, 'pitched')
  k.free()


@pytest.mark.gpu
@pytest.mark.skipif(HOSTEMU, reason='390 rows: beyond the host build\'s share')
def test_several_tiles_per_block_and_several_partials(nat, ctxs):
  """390 rows = 13 tiles: max_blocks = 2 gives 7 and 6 tiles per block and two partials, max_blocks = 0 one tile per block
  and 13 partials.  Both within tolerance of the reference; each is deterministic."""
  c = ctxs('point')
  prm, batch, shapes = _setup('point', 64, 390, 'relu', seed=11)
  coef = dict(G.COEF, scale=1.0 / 390)
  ref, tol, _ = _reference(prm, batch, coef, 'relu')
  out = []
  for mb in (2, 0):
    k = _Call(nat, c, P.pack(prm), batch, 64, 130, 3, coef, max_blocks=mb)
    assert k.run() == 0, c.lib.sag_last_error(c.h)
    out.append(k.grad())
    _check(out[-1], shapes, ref, tol, f'max_blocks {mb}')
    k.fill(SENTINEL)
    assert k.run() == 0
    np.testing.assert_array_equal(k.grad().view(np.uint32), out[-1].view(np.uint32), err_msg='two calls differ')
    k.free()


@pytest.mark.gpu
def test_directed_cases_are_exact(nat, ctxs):
  c = ctxs('car')
  od, nu = ROBOTS['car']
  H, n = 32, 65
  prm, batch, shapes = _setup('car', H, n, 'relu', seed=21)
  base = dict(G.COEF, scale=1.0 / n)

  def run(coef, b=batch, params=prm, drop=()):
    k = _Call(nat, c, P.pack(params), b, H, n, 1, coef, drop=drop)
    assert k.run() == 0, c.lib.sag_last_error(c.h)
    w = k.grad()
    k.free()
    return w

  def mean_part_is_zero(w):
    g, _ = G.split(w, shapes)
    return (g['W3'][:, :nu] == 0).all() and (g['b3'][:nu] == 0).all() and (g['std'] == 0).all()

  # no actor term at all
  w = run(dict(base, adv_mul=0.0, cadv_mul=0.0, ent_coef=0.0))
  assert mean_part_is_zero(w) and np.abs(G.split(w, shapes)[0]['W3'][:, nu]).max() > 0
  # every row clipped with the adverse sign: rho = 1.5 under a positive advantage
  lp = G.logp64(prm, batch['obs'], batch['actions'])
  clipped = dict(batch, logp_old=(lp - np.log(1.5)).astype(F32), adv=(np.abs(batch['adv']) + F32(0.1)).astype(F32))
  w = run(dict(base, cadv_mul=0.0, ent_coef=0.0), clipped)
  st = G.split(w, shapes)[1]
  assert mean_part_is_zero(w) and st[4] == st[5] > 0
  # no reward critic
  g, _ = G.split(run(dict(base, vf_coef=0.0)), shapes)
  assert (g['W3'][:, nu] == 0).all() and g['b3'][nu] == 0 and np.abs(g['W3'][:, nu + 1]).max() > 0
  # absent cost arrays are zero coefficients, bit for bit (statistic 2 is the one word that may differ: it is absent too)
  a = run(dict(base, cadv_mul=0.0, cvf_coef=0.0))
  b = run(base, drop=('cadv', 'cret'))
  keep = np.ones(len(a), bool)
  keep[len(a) - 8 + 2] = False
  np.testing.assert_array_equal(a.view(np.uint32)[keep], b.view(np.uint32)[keep])
  assert b[len(b) - 8 + 2] == 0
  # zero weights, nonzero biases
  zero = {k_: (np.zeros_like(v) if k_[0] == 'W' else v) for k_, v in prm.items()}
  ref, tol, _ = _reference(zero, batch, base, 'relu')
  _check(run(base, params=zero), shapes, ref, tol, 'zero weights')
  # scale doubled doubles every word
  np.testing.assert_array_equal(run(dict(base, scale=2.0 / n)), 2 * run(base))


@pytest.mark.gpu
def test_accumulate_adds_the_other_planes(nat, ctxs):
  c = ctxs('point')
  H, rows, planes = 64, 33, 3
  prm, batch, shapes = _setup('point', H, rows * planes, 'tanh', seed=31)
  coef = dict(G.COEF, scale=1.0 / (rows * planes))
  ref, tol, _ = _reference(prm, batch, coef, 'tanh')
  k = _Call(nat, c, P.pack(prm), batch, H, rows, planes, coef, 'tanh')
  assert k.run() == 0
  whole = k.grad()
  # the same call, accumulating from a zeroed buffer: equal bits
  k.c.dev_upload(k.p['grad'], np.concatenate([np.zeros(k.n_words, F32), np.full(GUARD, SENTINEL, F32)]))
  k.desc.flags = ACCUMULATE
  assert k.run() == 0
  np.testing.assert_array_equal(k.grad().view(np.uint32), whole.view(np.uint32))
  # plane 0, then planes 1 and 2 on top of it
  k.fill(SENTINEL)
  k.desc.flags, k.desc.n_planes = 0, 1
  assert k.run() == 0
  k.desc.flags, k.desc.n_planes = ACCUMULATE, 2
  for name in INPUTS:
    per_row = k.host[name][0, 0].size * 4
    setattr(k.desc, 'd_' + name, k.p[name].value + k.pitch * per_row)
  assert k.run() == 0
  _check(k.grad(), shapes, ref, tol, 'plane 0 + planes 1, 2')
  assert k.inputs_unchanged()
  k.free()


@pytest.mark.gpu
def test_refusals_enqueue_nothing(nat, ctxs):
  c = ctxs('point')
  prm, batch, shapes = _setup('point', 32, 33, 'relu', seed=41)
  coef = dict(G.COEF, scale=1.0 / 33)
  k = _Call(nat, c, P.pack(prm), batch, 32, 33, 1, coef)
  good = {f: getattr(k.desc, f) for f, _ in k.desc._fields_}

  def refused(code=ERR_ARG, **change):
    for f, v in good.items():
      setattr(k.desc, f, v)
    for f, v in change.items():
      setattr(k.desc, f, v)
    rc = k.run()
    assert rc == code, (change, rc)
    assert (k.words() == F32(SENTINEL)).all(), f'{change}: d_grad was written'
    assert c.lib.sag_last_error(c.h)

  for f in ('d_params', 'd_obs', 'd_actions', 'd_logp_old', 'd_adv', 'd_ret', 'd_grad'):
    refused(**{f: None})
  refused(d_obs=good['d_obs'] + 4)
  for f in ('d_params', 'd_actions', 'd_logp_old', 'd_adv', 'd_ret', 'd_cadv', 'd_cret', 'd_grad'):
    refused(**{f: good[f] + 2})
  for h in (0, 16, 48, 288, -32):
    refused(hidden=h)
  for h in (160, 192, 224, 256):
    refused(ERR_UNSUPPORTED, hidden=h)
  assert b'128' in c.lib.sag_last_error(c.h)
  refused(activation=2)
  refused(flags=2)
  refused(obs_pitch=56)
  refused(obs_pitch=62)
  refused(n_rows=0)
  refused(n_planes=0)
  refused(pitch=32)
  refused(max_blocks=-1)
  for clip in (0.0, 1.0, -0.2, float('nan')):
    refused(clip=clip)
  for f in ('vf_coef', 'cvf_coef', 'ent_coef', 'adv_mul', 'adv_sub', 'cadv_mul', 'cadv_sub', 'scale'):
    refused(**{f: float('inf')})
    refused(**{f: float('nan')})
  assert c.lib.sag_policy_backward_device(c.h, None) == ERR_ARG
  assert c.lib.sag_policy_backward_device(None, None) == ERR_ARG
  for f, v in good.items():
    setattr(k.desc, f, v)
  assert k.run() == 0   # the context is usable after the refusals
  assert np.isfinite(k.grad()).all()
  # Adam's
  n = 8
  buf = {x: c.dev_alloc(4 * n + 8) for x in 'pgmv'}
  for b in buf.values():
    c.dev_upload(b, np.full(n + 2, SENTINEL, F32))
  ok = dict(n=n, clamp_first=n, beta1=0.9, beta2=0.999, eps=1e-8, step=1e-3, clamp_lo=0.0, reserved=0.0,
            d_param=buf['p'].value, d_grad=buf['g'].value, d_m=buf['m'].value, d_v=buf['v'].value)
  bad = [dict(n=0), dict(clamp_first=-1), dict(clamp_first=n + 1), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float('nan')),
         dict(eps=0.0), dict(eps=-1e-8), dict(step=float('inf')), dict(clamp_lo=float('nan'))]
  bad += [{f: None} for f in ('d_param', 'd_grad', 'd_m', 'd_v')] + [{f: ok[f] + 2} for f in ('d_param', 'd_grad', 'd_m', 'd_v')]
  for change in bad:
    d = nat.AdamDesc(**dict(ok, **change))
    assert c.lib.sag_adam_device(c.h, C.byref(d)) == ERR_ARG, change
    c.wait()
    assert all((c.dev_download(b, (n + 2,), F32) == F32(SENTINEL)).all() for b in buf.values()), change
  assert c.lib.sag_adam_device(c.h, None) == ERR_ARG
  for b in buf.values():
    c.dev_free(b)
  k.free()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 8324])
def test_adam_equals_the_float32_chain_bit_for_bit(nat, ctxs, n):
  """Three consecutive steps on the device's own gradient of a Point batch (hidden 64: 8326 words, of which the first n are
  taken), with a zero and a denormal planted in it, for clamp_first in {0, n - 2, n}."""
  c = ctxs('point')
  prm, batch, shapes = _setup('point', 64, 33, 'relu', seed=51)
  flat = P.pack(prm)
  assert len(flat) == 8326
  k = _Call(nat, c, flat, batch, 64, 33, 1, dict(G.COEF, scale=1.0 / 33))
  assert k.run() == 0
  g = k.grad()[:n].copy()
  k.free()
  g[0] = 0.0
  g[-1] = F32(1e-41)
  assert n == 1 or (g[-1] != 0 and abs(g[-1]) < np.finfo(F32).tiny)
  for first in sorted({0, max(n - 2, 0), n}):
    p, m, v = flat[:n].copy(), np.zeros(n, F32), np.zeros(n, F32)
    d = {x: c.dev_alloc(4 * (n + 2)) for x in 'pgmv'}
    for x, a in zip('pgmv', (p, g, m, v)):
      c.dev_upload(d[x], np.concatenate([a, np.full(2, SENTINEL, F32)]))
    lo = 0.05
    for t in (1, 2, 3):
      step = G.adam_step_size(3e-3, t)
      c.adam(n, d['p'], d['g'], d['m'], d['v'], step, clamp_first=first, clamp_lo=lo)
      p, m, v = G.adam_ref32(p, g, m, v, step, clamp_first=first, clamp_lo=lo)
      c.wait()
      for x, want in zip('pmv', (p, m, v)):
        got = c.dev_download(d[x], (n + 2,), F32)
        np.testing.assert_array_equal(got[:n].view(np.uint32), want.view(np.uint32), err_msg=f'{x} after step {t}, clamp_first {first}')
        assert (got[n:] == F32(SENTINEL)).all()
    assert (p[first:] >= F32(lo)).all()
    assert (c.dev_download(d['g'], (n,), F32).view(np.uint32) == g.view(np.uint32)).all()
    for b in d.values():
      c.dev_free(b)


# ----------------------------------------------------------------------------------------------------------------------
# sag.PPOLearner with sag.MLPPolicy and sag.RolloutBuffer
# ----------------------------------------------------------------------------------------------------------------------
def _loop(seed=3):
  import safe_adaptation_gym_amd as sag
  from test_reset_loop import _make_env
  env = _make_env('point', 'go_to_goal', n_envs=64, seed=seed, device_buffers=True, time_limit=5, auto_reset=True)
  env.reset()
  pi = sag.MLPPolicy(env, hidden=32, activation='tanh', seed=1)
  buf = sag.RolloutBuffer(env, steps=8)
  buf.collect(pi)
  pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  return sag, env, pi, buf, out


def _host_batch(buf, out, t0, t1):
  get = lambda v: v.numpy()[t0:t1]   # noqa: E731
  n = (t1 - t0) * buf.N
  return dict(obs=get(buf.obs).reshape(n, -1), actions=get(buf.actions).reshape(n, -1), logp_old=get(buf.logp).reshape(n),
              adv=get(out['adv']).reshape(n), ret=get(out['ret']).reshape(n), cadv=get(out['cadv']).reshape(n), cret=get(out['cret']).reshape(n))


@pytest.mark.gpu
def test_learner_updates_the_policy_from_the_buffer_in_place(nat):
  """Point / go_to_goal, 64 envs, time limit 5, T = 8, hidden 32, tanh.  The gradient of the learner's first minibatch (planes
  0 ... 3, the very call update() makes first) equals the reference recomputed from the downloaded buffer and the parameters
  before the update, under the tolerance of the module's docstring; after update() the parameters moved, are finite, std is at
  or above std_min and the policy's constant belongs to the new std."""
  from safe_adaptation_gym_amd.policy import plane_range
  sag, env, pi, buf, out = _loop()
  learner = sag.PPOLearner(pi, buf, epochs=2, minibatches=2, cost_weight=0.5, ent_coef=0.01, lr=1e-2, std_min=0.5)
  assert learner.ranges() == [(0, 4), (4, 8)]
  before = pi.get_params()
  t0, t1 = learner.ranges()[0]
  cut = lambda v: plane_range(v, t0, t1)   # noqa: E731
  coef = dict(clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.01, adv_mul=1.0, adv_sub=0.0, cadv_mul=0.5, cadv_sub=0.0, scale=1.0 / (4 * 64))
  pi.backward(cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(out['adv']), cut(out['ret']), cut(out['cadv']), cut(out['cret']),
              clip=0.2, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.01, cadv_affine=(0.5, 0.0), scale=coef['scale'])
  buf.wait()
  words = np.concatenate([pi.grad[k].numpy().reshape(-1) for k in P.KEYS] + [pi.grad['stats'].numpy()])
  batch = _host_batch(buf, out, t0, t1)
  ref, tol, _ = _reference(before, batch, coef, 'tanh')
  _check(words, pi.shapes, ref, tol, 'first minibatch')
  assert set(pi.grad) == set(P.KEYS) | {'stats'} and all(pi.grad[k].shape == pi.shapes[k] for k in P.KEYS)
  stats = learner.update(out)
  assert learner.t == 4 and set(stats) == {'policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl', 'clip_fraction'}
  assert all(np.isfinite(v) for v in stats.values()) and 0 <= stats['clip_fraction'] <= 1
  after = pi.get_params()
  for k in P.KEYS:
    assert np.isfinite(after[k]).all() and (after[k] != before[k]).any(), k
  assert (after['std'] >= F32(0.5)).all()   # exp(-0.5) = 0.61 at the start, four steps of 1e-2 and a floor of 0.5
  assert pi.logp_const == P.logp_const(after['std'])
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, minibatches=9)
  with pytest.raises(ValueError):
    pi.backward(buf.obs, buf.actions, buf.logp, out['adv'], out['ret'], clip=0.2, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0,
                scale=1.0)   # obs has T + 1 planes
  learner.close(); pi.close(); buf.close()


@pytest.mark.gpu
def test_value_only_learner_fits_the_returns_of_a_fixed_batch(nat):
  """Zero advantages switch the surrogate off and vf_coef = 1 leaves the reward critic's loss: 30 updates (one round each) on
  one fixed batch must bring the value loss below half its first value.  Beforehand the float64 reference with adam_ref32 on
  the same batch, on the host, must reach below a quarter - the batch and the step size can do it."""
  sag, env, pi, buf, out = _loop()
  c = pi._ctx
  # Point's returns over 8 steps are a few hundredths and the fresh critic's outputs as small: the loss starts at its noise
  # floor.  The critic's bias is therefore moved off by one AFTER the returns were formed: something to learn.
  prm = pi.get_params()
  prm['b3'][2] += F32(1.0)
  pi.set_params(prm)
  c.dev_upload(nat.C.c_void_p(out['adv']._base[0]), np.zeros(out['adv']._base[1], F32))
  c.dev_upload(nat.C.c_void_p(out['cadv']._base[0]), np.zeros(out['cadv']._base[1], F32))
  lr = 5e-2
  batch = _host_batch(buf, out, 0, 8)
  assert not batch['adv'].any()
  coef = dict(clip=0.2, vf_coef=1.0, cvf_coef=0.0, ent_coef=0.0, adv_mul=1.0, adv_sub=0.0, cadv_mul=0.0, cadv_sub=0.0, scale=1.0 / 512)
  flat, m, v = P.pack(prm), np.zeros(pi.n_params, F32), np.zeros(pi.n_params, F32)
  losses = []
  for t in range(1, 31):
    now = G.split(flat, pi.shapes)[0]
    _, g, s = G.loss_grad64(now, batch, coef, None, 'tanh')
    losses.append(s[1])
    flat, m, v = G.adam_ref32(flat, G.flat(g, s)[:pi.n_params].astype(F32), m, v, G.adam_step_size(lr, t), clamp_first=pi.n_params - 2,
                              clamp_lo=1e-3)
  print(f'reference value loss {losses[0]:.4f} -> {losses[-1]:.4f}')
  assert losses[-1] < 0.25 * losses[0]
  learner = sag.PPOLearner(pi, buf, lr=lr, epochs=1, minibatches=1, vf_coef=1.0, cost_vf_coef=0.0)
  seen = [learner.update(out)['value_loss'] for _ in range(30)]
  print(f'device value loss {seen[0]:.4f} -> {seen[-1]:.4f}')
  assert abs(seen[0] - losses[0]) <= 1e-5 * losses[0]   # the same 512 terms, summed in fp32
  assert seen[-1] < 0.5 * seen[0]
  learner.close(); pi.close(); buf.close()

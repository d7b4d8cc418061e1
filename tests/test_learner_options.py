"""sag.PPOLearner with advantage normalisation, gradient clipping and the device-side Lagrange multiplier switched on
(learner.py over csrc/sag_learner.hpp): Point / go_to_goal, hidden 32, tanh, T = 8, 33 envs (a pitch of 256: 223 pad rows per
plane), time limit 5 so that every env ends an episode inside the buffer, 2 epochs x 3 minibatches.

update() is compared with a twin composed by hand from the Context methods in the order learner.py documents - moments of adv
and cadv, moments of the ended episodes' costs, the multiplier's step, the mix, then per round backward, clip, Adam - on words
and a mixed array of the test's own.  Everything the twin leaves equals what update() left, bit for bit; along the way the
device's moments are within the kernels' tolerance of the float64 restatement (tests/learner_ref.py), the mixed advantage equals
mix32 on the device's own moments, the clipped gradient equals scale32 of the device's own gradient and factor, and Adam equals
adam_ref32 on that clipped gradient."""
import numpy as np
import pytest

import learner_ref as R
import policy_grad_ref as G
import policy_ref as P

F32, F64 = np.float32, np.float64
FACTOR = 8.0
N_ENVS, T = 33, 8
ADV_MOM, CADV_MOM, EP_MOM, LAG, CLIP, WORDS = 0, 4, 8, 12, 16, 20
BASE = dict(epochs=2, minibatches=3, cost_weight=0.3, ent_coef=0.01, lr=1e-2, std_min=0.5)
OPTIONS = dict(normalize_advantage=True, max_grad_norm=0.05, cost_budget=0.5, lagrange_lr=0.05, lagrange_max=10.0)
STATS = {'policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl', 'clip_fraction'}


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


def _loop(seed=3):
  import safe_adaptation_gym_amd as sag
  from test_reset_loop import _make_env
  env = _make_env('point', 'go_to_goal', n_envs=N_ENVS, seed=seed, device_buffers=True, time_limit=5, auto_reset=True)
  env.reset()
  pi = sag.MLPPolicy(env, hidden=32, activation='tanh', seed=1)
  buf = sag.RolloutBuffer(env, steps=T)
  buf.collect(pi)
  pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  return sag, env, pi, buf, out


def _words(c, ptr, n):
  c.wait()
  return c.dev_download(ptr, (n,), F32)


def _within(got, values, what):
  ref = R.moments64(values, 1e-8)
  own = R.moments_measure(R.moments32(values, 1e-8), ref)
  m = R.moments_measure(got, ref)
  tol = FACTOR * max(own.values())
  print(f'{what}: tolerance {tol:.3e}, device ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
  assert got[0] == ref[0] and all(v <= tol for v in m.values()), (what, m, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('cost,cost_advantage', [(True, 'center'), (True, 'standardize'), (False, 'center')])
def test_update_with_every_switch_on_equals_its_composed_twin(nat, cost, cost_advantage):
  from safe_adaptation_gym_amd.policy import plane_range
  sag, env, pi, buf, out = _loop()
  if not cost:
    out = {k: out[k] for k in ('adv', 'ret')}
  c, n, nu, N, Pt = pi._ctx, pi.n_params, pi.nu, buf.N, buf.P
  assert (N, Pt) == (33, 256)
  before = pi.get_params()
  learner = sag.PPOLearner(pi, buf, cost_advantage=cost_advantage, **BASE, **OPTIONS)
  ranges = [(0, 2), (2, 5), (5, 8)]
  assert learner.ranges() == ranges and learner.cost_weight == 0.3
  stats = learner.update(out)
  after = pi.get_params()
  left = _words(c, learner._words, WORDS)
  left_mixed = _words(c, learner._mixed, T * Pt).reshape(T, Pt).copy()
  assert learner.t == 6

  # the twin
  pi.set_params(before)
  adv = out['adv'].numpy()
  done = buf.done.numpy()
  ep_cost = buf.episode.numpy()[..., 1]
  assert adv.shape == (T, N) and np.count_nonzero(done) >= N   # every env met its time limit of 5 inside 8 steps
  dw, dmix = c.dev_alloc(WORDS * 4), c.dev_alloc(T * Pt * 4)
  state0 = np.zeros(WORDS, F32)
  state0[LAG] = 0.3
  c.dev_upload(dw, state0)
  c.dev_upload(dmix, np.full(T * Pt, 7.0, F32))
  w = lambda k: dw.value + 4 * k   # noqa: E731
  cadv_mode = {'center': 1, 'standardize': 2}[cost_advantage] if cost else 0
  c.moments(N, T, Pt, out['adv'].ptr, w(ADV_MOM), eps=1e-8)
  if cost:
    c.moments(N, T, Pt, out['cadv'].ptr, w(CADV_MOM), eps=1e-8)
  c.moments(N, T, Pt, buf.episode.ptr + 4, w(EP_MOM), d_mask=buf.done.ptr, stride=4, eps=1e-8)
  c.lagrange(w(EP_MOM), w(LAG), 0.05, 0.5, 10.0)
  c.advantage_mix(N, T, Pt, out['adv'].ptr, dmix, d_cadv=out['cadv'].ptr if cost else None, adv_mode=2, cadv_mode=cadv_mode,
                  d_adv_mom=w(ADV_MOM), d_cadv_mom=w(CADV_MOM), d_lambda=w(LAG), cost_weight=0.3)
  words = _words(c, dw, WORDS)
  _within(words[ADV_MOM:ADV_MOM + 4], adv.reshape(-1), 'adv')
  cadv = out['cadv'].numpy() if cost else None
  if cost:
    _within(words[CADV_MOM:CADV_MOM + 4], cadv.reshape(-1), 'cadv')
  else:
    assert not words[CADV_MOM:CADV_MOM + 4].any()
  _within(words[EP_MOM:EP_MOM + 4], ep_cost[done != 0], 'episode costs')
  assert words[EP_MOM] == np.count_nonzero(done)
  lag = R.lagrange32([0.3, 0, 0, 0], words[EP_MOM:EP_MOM + 4], 0.05, 0.5, 10.0)
  assert words[LAG:LAG + 4].tobytes() == lag.tobytes() and lag[3] == 1 and lag[0] != F32(0.3)
  mixed = _words(c, dmix, T * Pt).reshape(T, Pt)
  want = R.mix32(adv, cadv, 2, cadv_mode, words[ADV_MOM:ADV_MOM + 4], words[CADV_MOM:CADV_MOM + 4], lag[0])
  assert mixed[:, :N].tobytes() == want.tobytes() and (mixed[:, N:] == F32(7.0)).all()
  assert left_mixed[:, :N].tobytes() == want.tobytes()

  mview = type(out['adv'])(c, dmix.value, (T, N), np.float32, strides=(Pt * 4, 4), base=(dmix.value, (T, Pt)))
  dm, dv = c.dev_alloc(4 * n), c.dev_alloc(4 * n)
  c.dev_upload(dm, np.zeros(n, F32))
  c.dev_upload(dv, np.zeros(n, F32))
  m, v = np.zeros(n, F32), np.zeros(n, F32)
  t, last, clipped = 0, None, 0
  for epoch in range(2):
    for t0, t1 in ranges:
      t += 1
      now = pi.get_params()
      cut = lambda x: plane_range(x, t0, t1)   # noqa: E731
      pi.backward(cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(mview), cut(out['ret']), None, cut(out['cret']) if cost else None,
                  clip=0.2, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.01, adv_affine=(1.0, 0.0), cadv_affine=(0.0, 0.0),
                  scale=1.0 / ((t1 - t0) * N))
      raw = _words(c, pi._gbuf, n + 8)
      c.grad_clip(n, pi._gbuf, w(CLIP), 0.05)
      got = _words(c, pi._gbuf, n + 8)
      norm, factor = _words(c, dw, WORDS)[CLIP:CLIP + 2]
      n64, _ = R.clip64(raw[:n], 0.05)
      own = abs(F64(R.clip32(raw[:n], 0.05)[0]) - n64) / n64
      print(f'round {t}: norm {norm:.4f} factor {factor:.4f}, norm error {abs(norm - n64) / n64:.2e} under {FACTOR * own:.2e}')
      assert abs(norm - n64) / n64 <= FACTOR * own
      assert factor == (F32(1) if F32(0.05) / F32(norm + F32(1e-6)) > 1 else F32(F32(0.05) / F32(norm + F32(1e-6))))
      assert got[:n].tobytes() == R.scale32(raw[:n], factor).tobytes() and got[n:].tobytes() == raw[n:].tobytes()
      clipped += factor < 1
      c.adam(n, pi._buf, pi._gbuf, dm, dv, learner.step_size(t), clamp_first=n - nu, clamp_lo=0.5)
      p, m, v = G.adam_ref32(P.pack(now), got[:n], m, v, G.adam_step_size(1e-2, t), clamp_first=n - nu, clamp_lo=0.5)
      for name, ptr, ref in (('parameters', pi._buf, p), ('m', dm, m), ('v', dv, v)):
        np.testing.assert_array_equal(_words(c, ptr, n).view(np.uint32), ref.view(np.uint32), err_msg=f'{name} after round {t}')
      last = got[n:]
  assert clipped >= 1, 'max_grad_norm = 0.05 never clipped: the clip path was not exercised'
  twin = pi.get_params()
  for k in P.KEYS:
    np.testing.assert_array_equal(twin[k].view(np.uint32), after[k].view(np.uint32), err_msg=f'{k}: update() against its twin')
    assert (after[k] != before[k]).any(), k
  for name, ptr in (('m', learner._m), ('v', learner._v)):
    np.testing.assert_array_equal(_words(c, ptr, n).view(np.uint32), {'m': m, 'v': v}[name].view(np.uint32), err_msg=f'the learner\'s {name}')
  final = _words(c, dw, WORDS)
  assert final.tobytes() == left.tobytes()
  assert stats == dict(policy_loss=float(last[0]), value_loss=float(last[1]), cost_value_loss=float(last[2]), approx_kl=float(last[3]),
                       clip_fraction=float(last[4] / last[5]), grad_norm=float(left[CLIP]), adv_mean=float(left[ADV_MOM + 1]),
                       adv_std=float(np.sqrt(left[ADV_MOM + 2])), cost_weight=float(left[LAG]), episode_cost=float(left[LAG + 1]),
                       episodes=int(np.count_nonzero(done)))
  assert learner.cost_weight == float(lag[0])
  if not cost:
    assert stats['cost_value_loss'] == 0.0
  for ptr in (dw, dmix, dm, dv):
    c.dev_free(ptr)
  learner.close(); pi.close(); buf.close()


@pytest.mark.gpu
def test_each_switch_alone_adds_only_its_own_keys(nat):
  """No switch: today's five keys and a cost_weight that stays a plain attribute.  One switch: the five and its own.  With
  cost_budget an assignment to cost_weight reaches the device word; a second update() steps the multiplier again."""
  sag, env, pi, buf, out = _loop()
  c = pi._ctx
  small = dict(epochs=1, minibatches=1, lr=1e-3)
  plain = sag.PPOLearner(pi, buf, cost_weight=0.25, **small)
  assert set(plain.update(out)) == STATS and plain.cost_weight == 0.25 and plain._words is None and plain._mixed is None
  plain.cost_weight = 0.5
  assert plain.cost_weight == 0.5
  plain.close()
  for kw, extra in ((dict(normalize_advantage=True), {'adv_mean', 'adv_std'}), (dict(max_grad_norm=0.5), {'grad_norm'}),
                    (dict(cost_budget=0.5), {'cost_weight', 'episode_cost', 'episodes'})):
    learner = sag.PPOLearner(pi, buf, cost_weight=0.25, **small, **kw)
    stats = learner.update(out)
    assert set(stats) == STATS | extra, (kw, set(stats))
    assert all(np.isfinite(x) for x in stats.values())
    if 'adv_std' in stats:
      a = out['adv'].numpy().astype(F64)
      assert abs(stats['adv_mean'] - a.mean()) <= 1e-5 * a.std() and abs(stats['adv_std'] - a.std()) <= 1e-5 * a.std()
    if 'episodes' in stats:
      done = buf.done.numpy()
      costs = buf.episode.numpy()[..., 1][done != 0]
      assert stats['episodes'] == np.count_nonzero(done) > 0
      first = R.lagrange32([0.25, 0, 0, 0], R.moments32(costs, 1e-8), 0.05, 0.5)
      assert abs(stats['cost_weight'] - R.lagrange64(0.25, costs.astype(F64).mean(), 0.05, 0.5)) <= 1e-6 * max(1.0, first[0])
      assert learner.cost_weight == stats['cost_weight']
      learner.cost_weight = 0.75
      assert _words(c, learner._words, WORDS)[LAG] == F32(0.75) and learner.cost_weight == 0.75
      again = learner.update(out)
      assert abs(again['cost_weight'] - R.lagrange64(0.75, costs.astype(F64).mean(), 0.05, 0.5)) <= 1e-6 * max(1.0, again['cost_weight'])
    learner.close()
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, cost_advantage='whiten')
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, max_grad_norm=0.0)
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, cost_budget=float('nan'))
  pi.close(); buf.close()

"""sag.PPOLearner(shuffle=True) (learner.py over csrc/sag_shuffle.hpp and the ROWS instances of csrc/sag_policy_grad.hpp):
Point / go_to_goal, hidden 32, tanh, 64 envs, T = 8 - 512 rows -, 2 epochs x 3 minibatches of 170, 171 and 171 rows.

update() is compared with a twin composed by hand from the Context methods: per epoch one permutation into an index array of
the test's own, then per minibatch the rows backward over a slice of it and Adam - and, with normalize_advantage, the moments
and the mix ahead of the rounds, as test_learner_options.py composes them.  Parameters and Adam moments equal update()'s bit
for bit; the learner's index array equals the NumPy restatement (tests/shuffle_ref.py) of the last epoch's permutation."""
import numpy as np
import pytest

import policy_ref as P
import shuffle_ref as S
from test_device_reset import KEY

F32 = np.float32
N_ENVS, T = 64, 8
BASE = dict(epochs=2, minibatches=3, cost_weight=0.3, ent_coef=0.01, lr=1e-2, std_min=0.5)


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def loop(nat):
  """One rollout shared by the tests: (sag, pi, buf, out, the parameters before any update).  The context key is KEY."""
  import safe_adaptation_gym_amd as sag
  from test_reset_loop import _make_env
  env = _make_env('point', 'go_to_goal', n_envs=N_ENVS, seed=3, device_buffers=True, time_limit=5, auto_reset=True)
  env.reset()
  pi = sag.MLPPolicy(env, hidden=32, activation='tanh', seed=1)
  buf = sag.RolloutBuffer(env, steps=T)
  buf.collect(pi)
  pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  pi._ctx.set_seed(KEY)
  yield sag, pi, buf, out, pi.get_params()
  pi.close(); buf.close()


def _words(c, ptr, n, dtype=F32):
  c.wait()
  return c.dev_download(ptr, (n,), dtype)


def _state(c, pi, learner):
  n = pi.n_params
  return {'p': _words(c, pi._buf, n), 'm': _words(c, learner._m, n), 'v': _words(c, learner._v, n)}


def _same(a, b, what):
  for k in a:
    np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f'{what}: {k}')


@pytest.mark.gpu
@pytest.mark.parametrize('normalize,cost', [(False, True), (True, True), (False, False)])
def test_shuffled_update_equals_its_composed_twin(nat, loop, normalize, cost):
  sag, pi, buf, out, before = loop
  if not cost:
    out = {k: out[k] for k in ('adv', 'ret')}
  c, n, nu, N, Pt = pi._ctx, pi.n_params, pi.nu, buf.N, buf.P
  total = T * N
  assert N == 64 and Pt >= N and total == 512
  pi.set_params(before)
  learner = sag.PPOLearner(pi, buf, normalize_advantage=normalize, shuffle=True, shuffle_draw=0xfffffffe, **BASE)
  stats = learner.update(out)
  assert learner.t == 6 and learner.shuffle_draw == 0   # two epochs from 0xfffffffe: the draw wraps at 2^32
  left = _state(c, pi, learner)
  # the learner's index array holds the last epoch's permutation
  index = _words(c, learner._index, total, np.int32)
  assert index.tobytes() == S.permutation(total, 0xffffffff, KEY).tobytes()
  assert np.array_equal(np.sort(index), np.arange(total))

  # the twin
  pi.set_params(before)
  didx, dm, dv = c.dev_alloc(total * 4), c.dev_alloc(4 * n), c.dev_alloc(4 * n)
  c.dev_upload(dm, np.zeros(n, F32))
  c.dev_upload(dv, np.zeros(n, F32))
  adv_ptr, cadv_ptr, affine = out['adv'].ptr, out['cadv'].ptr if cost else None, (0.3, 0.0)
  free = [didx, dm, dv]
  if normalize:   # moments of adv and cadv, then the mix: adv standardised, cadv centred, lambda = cost_weight
    dw, dmix = c.dev_alloc(8 * 4), c.dev_alloc(T * Pt * 4)
    free += [dw, dmix]
    c.dev_upload(dw, np.zeros(8, F32))
    c.moments(N, T, Pt, adv_ptr, dw.value, eps=1e-8)
    if cost:
      c.moments(N, T, Pt, cadv_ptr, dw.value + 16, eps=1e-8)
    c.advantage_mix(N, T, Pt, adv_ptr, dmix, d_cadv=cadv_ptr, adv_mode=2, cadv_mode=1 if cost else 0, d_adv_mom=dw.value,
                    d_cadv_mom=dw.value + 16, cost_weight=0.3)
    adv_ptr, cadv_ptr, affine = dmix.value, None, (0.0, 0.0)
  edges = [total * m // 3 for m in range(4)]
  assert edges == [0, 170, 341, 512]
  t, last = 0, None
  for epoch in range(2):
    c.permutation(total, (0xfffffffe + epoch) & 0xffffffff, didx)
    for a, b in zip(edges[:-1], edges[1:]):
      t += 1
      c.policy_backward(N, T, Pt, 32, pi._buf, buf.obs.ptr, buf.actions.ptr, buf.logp.ptr, adv_ptr, out['ret'].ptr, pi._gbuf, 1.0 / (b - a),
                        d_cadv=cadv_ptr, d_cret=out['cret'].ptr if cost else None, clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.01,
                        adv_affine=(1.0, 0.0), cadv_affine=affine, activation=nat.POLICY_TANH, rows=(didx.value + 4 * a, b - a))
      last = _words(c, pi._gbuf, n + 8)
      assert abs(last[n + 5] - 1.0) < 1e-6, 'statistic 5: every entry of the slice took part'
      c.adam(n, pi._buf, pi._gbuf, dm, dv, learner.step_size(t), clamp_first=n - nu, clamp_lo=0.5)
  twin = {'p': _words(c, pi._buf, n), 'm': _words(c, dm, n), 'v': _words(c, dv, n)}
  _same(twin, left, 'update() against its twin')
  assert (left['p'] != P.pack(before)).any() and np.isfinite(left['p']).all()
  assert _words(c, didx, total, np.int32).tobytes() == index.tobytes()
  for key, want in zip(('policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl'), last[n:n + 4]):
    assert stats[key] == float(want), key
  assert stats['clip_fraction'] == float(last[n + 4] / last[n + 5])
  for p in free:
    c.dev_free(p)
  learner.close()


@pytest.mark.gpu
def test_shuffle_false_is_the_learner_without_the_keyword(nat, loop):
  sag, pi, buf, out, before = loop
  c = pi._ctx
  got = []
  for kw in ({}, dict(shuffle=False), dict(shuffle=False, shuffle_draw=9)):
    pi.set_params(before)
    learner = sag.PPOLearner(pi, buf, **BASE, **kw)
    assert learner._index is None and learner.ranges() == [(0, 2), (2, 5), (5, 8)]
    learner.update(out)
    assert learner.shuffle_draw == kw.get('shuffle_draw', 0)   # nothing was drawn
    got.append(_state(c, pi, learner))
    learner.close()
  _same(got[1], got[0], 'shuffle=False')
  _same(got[2], got[0], 'shuffle=False, shuffle_draw=9')
  # and the shuffled update is another one
  pi.set_params(before)
  learner = sag.PPOLearner(pi, buf, shuffle=True, **BASE)
  learner.update(out)
  assert (_state(c, pi, learner)['p'] != got[0]['p']).any()
  learner.close()


@pytest.mark.gpu
def test_minibatches_beyond_T_need_shuffle(nat, loop):
  sag, pi, buf, out, before = loop
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, minibatches=T + 1)
  with pytest.raises(ValueError):
    sag.PPOLearner(pi, buf, minibatches=T * N_ENVS + 1, shuffle=True)
  pi.set_params(before)
  learner = sag.PPOLearner(pi, buf, epochs=1, minibatches=T + 1, shuffle=True, lr=1e-3)
  stats = learner.update(out)
  assert learner.t == T + 1 and all(np.isfinite(v) for v in stats.values())
  learner.close()


@pytest.mark.gpu
def test_draw_advances_by_epochs_and_a_restart_reproduces_the_next_update(nat, loop):
  sag, pi, buf, out, before = loop
  c = pi._ctx
  pi.set_params(before)
  a = sag.PPOLearner(pi, buf, shuffle=True, shuffle_draw=5, **BASE)
  a.update(out)
  assert a.shuffle_draw == 5 + BASE['epochs']
  saved = dict(params=pi.get_params(), m=_words(c, a._m, pi.n_params), v=_words(c, a._v, pi.n_params), t=a.t, draw=a.shuffle_draw)
  a.update(out)
  assert a.shuffle_draw == 5 + 2 * BASE['epochs']
  want = _state(c, pi, a)
  a.close()
  # a learner restarted from the checkpoint: parameters, moments, step count and the draw
  pi.set_params(saved['params'])
  b = sag.PPOLearner(pi, buf, shuffle=True, shuffle_draw=saved['draw'], **BASE)
  c.dev_upload(b._m, saved['m'])
  c.dev_upload(b._v, saved['v'])
  b.t = saved['t']
  b.update(out)
  _same(_state(c, pi, b), want, 'the restarted learner')
  # from another draw the same update differs
  pi.set_params(saved['params'])
  b.shuffle_draw = 1000
  c.dev_upload(b._m, saved['m'])
  c.dev_upload(b._v, saved['v'])
  b.t = saved['t']
  b.update(out)
  assert (_state(c, pi, b)['p'] != want['p']).any()
  b.close()


@pytest.mark.gpu
def test_backward_takes_a_device_view_or_a_pointer_pair(nat, loop):
  """MLPPolicy.backward(rows=): an int32 DeviceArray view and (pointer, count) name the same list; a float view, a
  two-dimensional one and an empty pair are refused before a kernel can read them."""
  sag, pi, buf, out, before = loop
  from safe_adaptation_gym_amd.policy import plane_range
  c, n, total = pi._ctx, pi.n_params, T * N_ENVS
  pi.set_params(before)
  d = c.dev_alloc(total * 4)
  c.permutation(total, 11, d)
  views = [plane_range(v, 0, T) for v in (buf.obs, buf.actions, buf.logp, out['adv'], out['ret'], out['cadv'], out['cret'])]
  kw = dict(clip=0.2, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.01, cadv_affine=(0.3, 0.0), scale=1.0 / 100)
  pi.backward(*views, rows=(d.value + 4 * 7, 100), **kw)
  pair = _words(c, pi._gbuf, n + 8)
  pi.backward(*views, rows=(d, 100), **kw)            # a c_void_p: entries 0 ... 99, another list
  assert (_words(c, pi._gbuf, n + 8) != pair).any()
  pi.backward(*views, rows=nat.DeviceArray(c, d.value + 4 * 7, (100,), np.int32), **kw)
  view = _words(c, pi._gbuf, n + 8)
  np.testing.assert_array_equal(view.view(np.uint32), pair.view(np.uint32))
  assert abs(pair[n + 5] - 1.0) < 1e-6 and np.isfinite(pair).all()
  for bad in (nat.DeviceArray(c, d.value, (100,), np.float32), nat.DeviceArray(c, d.value, (10, 10), np.int32), (d.value, 0), (d.value + 2, 4)):
    with pytest.raises(ValueError):
      pi.backward(*views, rows=bad, **kw)
  # a normalising policy hands its table to the rows entry point: the identity list gives the bits of its contiguous backward
  pin = sag.MLPPolicy(pi.env, hidden=32, activation='tanh', seed=2, normalize_observations=True, obs_clip=5.0)
  pin.update_obs_stats(buf)
  c.dev_upload(d, np.arange(total, dtype=np.int32))
  kw['scale'] = 1.0 / total
  pin.backward(*views, **kw)
  want = _words(c, pin._gbuf, n + 8)
  pin.backward(*views, rows=(d, total), **kw)
  np.testing.assert_array_equal(_words(c, pin._gbuf, n + 8).view(np.uint32), want.view(np.uint32))
  pin.close()
  c.dev_free(d)

"""The loop a training run executes in throughput mode - step, step, ..., reset(mask), step, ... - as a whole: masked device
resets (sag_reset_device with a mask, csrc/sag_reset.hpp) in the middle of rollouts, checked against the other launch forms,
the NumPy restatement (tests/reset_sampler_ref.py), fresh contexts given the same records, and the CPU oracle.

What a masked reset must keep coherent besides the record (sag_api.hip): the hot records, the two busy-bit phases, the
alternating busy counters and the kinds, the cost bytes, the Doggo result block and its launch order, the layout store, the
generator's address (env id, episode nonce, step) and pending external contacts.  Every GPU test here also runs on the
sanitizer host build (tests/hostemu/run.sh) at reduced sizes."""
import os

import numpy as np
import pytest

import batch_util as bu
import render_ref as rr
import reset_sampler_ref as R
from test_device_reset import KEY, _assert_records, _cfg, _prev, _ref_batch

HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
ENV_ID0 = 5000
EPISODE0 = 41
CAR_TASKS = ['go_to_goal', 'push_box', 'press_buttons', 'unsupervised', 'catch_goal', 'haul_box']   # (test_gpu_parity.CAR_TASKS)
# point / haul_box with pillars and vases large enough that boxes are spawned over them often (the box sits at robot + .6
# with no keep-out check): R.install_awake of the restatement's records says how often (test_haul_box_config_...)
HAUL_CONFIG = {'pillars_size': 0.3, 'vases_size': 0.15}


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def oracle():
  from oracle_lib import Oracle
  return Oracle()


def _tid(name):
  from safe_adaptation_gym_amd import benchmark
  return benchmark.TASKS[name].TASK_ID


def _doggo_mix(n):
  from safe_adaptation_gym_amd import benchmark
  tids = np.array([_tid(nm) for nm, _ in benchmark.make('multitask', batch_size=n, seed=666).train_tasks])
  uniq, doe = np.unique(tids, return_inverse=True)
  return [int(t) for t in uniq], doe.astype(np.int32)


def _make(nat, robot, tids, n, doe=None, key=KEY, env_id0=ENV_ID0, config=None):
  """A context with its tasks set (env i: descriptor i mod len(tids) unless doe says otherwise); no layout yet."""
  descs = [nat.task_desc_default(t) for t in tids]
  doe = (np.arange(n) % len(tids)).astype(np.int32) if doe is None else np.asarray(doe, np.int32)
  c = nat.Context(robot, n, seed=key)
  c.set_tasks(descs, doe, config, env_id0=env_id0)
  return c, descs, doe


class _DevMask:
  """A device buffer of one context that carries host masks to sag_reset_device."""

  def __init__(self, c):
    self.c, self.p = c, c.dev_alloc(c.n_envs)

  def __call__(self, m):
    m = np.ascontiguousarray(m, np.uint8)
    assert m.shape == (self.c.n_envs,)
    self.c.dev_upload(self.p, m)
    return self.p

  def free(self):
    self.c.dev_free(self.p)


def _same(a, b, what):
  for k, (x, y) in enumerate(zip(a, b)):
    np.testing.assert_array_equal(x, y, err_msg=f'{what} [{k}]')


def _expect_reset(robot, descs, doe, cfg, gids, key, pre, post, m):
  """The rows `m` of `post` are the restatement's later-episode records of nonce + 1 drawn on top of `pre`; the rest of `post`
  is `pre`, in floats and ints."""
  (f0, i0), (f1, i1) = pre, post
  np.testing.assert_array_equal(f1[~m], f0[~m], err_msg='floats of an env outside the mask changed')
  np.testing.assert_array_equal(i1[~m], i0[~m], err_msg='ints of an env outside the mask changed')
  if not m.any():
    return
  nonce = (i0[m, R.I_EPISODE].astype(np.int64) + 1) & 0xffffff
  rf, ri, st = _ref_batch(robot, descs, doe[m], cfg, gids[m], nonce, key, False, _prev(f0[m], i0[m]))
  assert not st.any()
  _assert_records(f1[m], i1[m], rf, ri, maxulp=1)
  assert (i1[m, R.I_STEP] == 0).all()
  np.testing.assert_array_equal(i1[m, R.I_EPISODE], nonce)
  # what _assert_records leaves out is what the install computes: task.reset's `last` distances and the awake flags
  np.testing.assert_array_max_ulp(f1[m][:, 38:41], R.install_last(f1[m], i1[m]), maxulp=1)
  np.testing.assert_array_equal(i1[m, R.I_AWAKE], R.install_awake(f1[m], i1[m]))


def _install_twin(nat, robot, key, f, i):
  """The records given to a fresh context with sag_set_layout come back identical, `last` and awake flags included."""
  tw = nat.Context(robot, len(f), seed=key)
  tw.set_layout(f, i)
  tf, ti = tw.get_state()
  tw.close()
  np.testing.assert_array_equal(tf, f, err_msg='set_layout of the reset records: floats')
  np.testing.assert_array_equal(ti, i, err_msg='set_layout of the reset records: ints')


# masks of the schedule: name -> f(n, rng, last outputs) -> uint8 [n]
def _m_events(n, rng, out): return ((out[4] != 0) | (out[2] != 0)).astype(np.uint8)
def _m_random(n, rng, out): return (rng.rand(n) < 0.3).astype(np.uint8)
def _m_zeros(n, rng, out): return np.zeros(n, np.uint8)
def _m_ones(n, rng, out): return np.ones(n, np.uint8)
def _m_last(n, rng, out): return (np.arange(n) == n - 1).astype(np.uint8)
def _m_first(n, rng, out): return (np.arange(n) == 0).astype(np.uint8)
def _m_bytes(n, rng, out): return np.where(rng.rand(n) < 0.3, np.where(rng.rand(n) < 0.5, 2, 255), 0).astype(np.uint8)


# step -> mask applied after it.  Two consecutive steps twice: a reset right after the first, all-busy step of the one before
SCHEDULE = {10: _m_events, 11: _m_random, 25: _m_zeros, 26: _m_events, 40: _m_ones, 41: _m_events, 50: _m_last, 55: _m_events,
            60: _m_first, 70: _m_events, 78: _m_bytes, 85: _m_events}
TWIN_AFTER_RESET, TWIN_CONTROL, RENDER_AT, T_STEPS = (26, 78), (33,), (11, 78), 100
DOGGO_SCHEDULE = {4: _m_events, 5: _m_random, 11: _m_zeros, 12: _m_last, 13: _m_ones, 20: _m_first, 21: _m_bytes, 22: _m_events}
DOGGO_TWIN_AFTER_RESET, DOGGO_TWIN_CONTROL, DOGGO_RENDER_AT, DOGGO_T_STEPS = (5, 22), (14,), (5,), 28

CASES = {
    'point-mixed': ('point', lambda n: (list(range(14)), None), None),
    'car-push_box': ('car', lambda n: ([_tid('push_box')], None), None),
    'car-mixed': ('car', lambda n: ([_tid(t) for t in CAR_TASKS], None), None),
    'point-haul_box': ('point', lambda n: ([_tid('haul_box')], None), HAUL_CONFIG),
    'doggo-mixed': ('doggo', _doggo_mix, None),
}


def _forms(robot):
  """(environment of the context's creation) per launch form; the last one, created without any switch, is the control
  that skips the all-zeros call and takes the all-ones mask as an unmasked reset."""
  if robot == 'doggo':
    return [{'SAG_DOGGO_SCHED': '1'}, {'SAG_DOGGO_SCHED': '0'}, {}]
  return [{'SAG_SPLIT': '0'}, {'SAG_SPLIT': '1'}, {'SAG_SPLIT': '1', 'SAG_BUSY_KINDS': '1', 'SAG_BUSY_KINDS_MIN': '0'}, {}]


SWITCHES = ('SAG_SPLIT', 'SAG_BUSY_KINDS', 'SAG_BUSY_KINDS_MIN', 'SAG_DOGGO_SCHED', 'SAG_EARLY_FORK')


def _contexts(nat, monkeypatch, forms, robot, tids, n, doe, **kw):
  out = []
  for env in forms:
    for k in SWITCHES:
      monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    out.append(_make(nat, robot, tids, n, doe, **kw))
  for k in SWITCHES:
    monkeypatch.delenv(k, raising=False)
  return [o[0] for o in out], out[0][1], out[0][2]


def _actions(robot, f, i, rng, t):
  if robot == 'doggo':
    act = rng.uniform(-1, 1, size=(len(f), 12)).astype(np.float32)
    if t < 3:
      act[:] = 0   # let the robots land first
    return act
  return bu.pursuit_actions(f, i, rng, robot=robot)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(CASES))
def test_launch_forms_agree_across_masked_device_resets(nat, monkeypatch, case):
  """Section 1 of the issue: every launch form of the step (single, split, split with busy lists by kind; the Doggo with and
  without its longest-first order) runs the same rollout with masked device resets in it, bit for bit - and each reset is
  checked against the restatement, a fresh context given the reset records (install twin), a fresh context given the whole
  state (checkpoint twin, 5 further steps), the cost overlay, and a control context."""
  robot, pick, config = CASES[case]
  doggo = robot == 'doggo'
  n = (70 if HOSTEMU else 300) if doggo else (203 if HOSTEMU else 1500)
  assert n % 64 and n % 256
  schedule, twin_reset, twin_control, render_at, T = (
      (DOGGO_SCHEDULE, DOGGO_TWIN_AFTER_RESET, DOGGO_TWIN_CONTROL, DOGGO_RENDER_AT, DOGGO_T_STEPS) if doggo else
      (SCHEDULE, TWIN_AFTER_RESET, TWIN_CONTROL, RENDER_AT, T_STEPS))
  tids, doe = pick(n)
  forms = _forms(robot)
  ctxs, descs, doe = _contexts(nat, monkeypatch, forms, robot, tids, n, doe, config=config)
  main, control = ctxs[:-1], ctxs[-1]
  cfg = _cfg(**(config or {}))
  gids = ENV_ID0 + np.arange(n)
  masks = [_DevMask(c) for c in ctxs]
  for c in ctxs:
    rc, st, b = c.reset_device(True, episode0=EPISODE0)
    assert rc == 0 and not st.any()
  state = ctxs[0].get_state()
  rf, ri, st = _ref_batch(robot, descs, doe, cfg, gids, np.full(n, EPISODE0), KEY, True)
  _assert_records(*state, rf, ri, maxulp=1)
  for c in ctxs[1:]:
    _same(state, c.get_state(), 'state after the first reset')
  episode = np.full(n, EPISODE0, np.int64)
  rng = np.random.RandomState(3)
  twins = []   # [fresh context restored from get_state(), steps left to compare]
  event_masks = cost_events = met_events = awake_by_overlap = overlay_seen = overlay_cleared = resets_checked = 0
  for t in range(T):
    act = _actions(robot, *state, rng, t)
    outs = [c.step(act) for c in ctxs]   # throughput mode: the device draws its own noise and words
    state = ctxs[0].get_state()
    for k, c in enumerate(ctxs[1:], 1):
      _same(outs[0][:5], outs[k][:5], f'step {t}: outputs of form {forms[k]}')
      _same(state, c.get_state(), f'step {t}: state of form {forms[k]}')
    if not doggo:
      assert ctxs[1].busy_count() == ctxs[2].busy_count(), f'step {t}'
    for tw in twins:
      _same(outs[0][:5], tw[0].step(act)[:5], f'step {t}: outputs of the checkpoint twin')
      _same(state, tw[0].get_state(), f'step {t}: state of the checkpoint twin')
      tw[1] -= 1
      if not tw[1]:
        tw[0].close()
    twins = [tw for tw in twins if tw[1]]
    np.testing.assert_array_equal(state[1][:, R.I_EPISODE], episode, err_msg=f'step {t}: a step changed a nonce')
    cost_events += int(outs[0][2].sum())
    met_events += int(outs[0][4].sum())
    if t in schedule:
      kind = schedule[t]
      m8 = kind(n, rng, outs[0])
      m = m8 != 0
      event_masks += int(kind is _m_events and m.any())
      for c, dm in zip(ctxs, masks):
        if c is control and kind is _m_zeros:
          continue   # the next steps of the others must equal a run without the call
        if c is control and kind is _m_ones:
          rc, st, b = c.reset_device(False)
        else:
          rc, st, b = c.reset_device(False, d_mask=dm(m8))
        assert rc == 0 and not st.any(), f'reset after step {t}'
        post = c.get_state()
        np.testing.assert_array_equal(b, post[0][:, R.F_BOUND], err_msg='bound of every env is returned')
        if c is ctxs[0]:
          _expect_reset(robot, descs, doe, cfg, gids, KEY, state, post, m)
          first = post
        else:
          _same(first, post, f'reset after step {t}: state of form {forms[ctxs.index(c)]}')
      episode[m] = (episode[m] + 1) & 0xffffff
      if m.any():
        _install_twin(nat, robot, KEY, first[0][m], first[1][m])
        resets_checked += 1
      if case == 'point-haul_box':
        awake_by_overlap += int((first[1][m, R.I_AWAKE] & R.install_awake(first[0][m], first[1][m]) & (1 << 10) != 0).sum())
      if t in render_at:
        # the cost byte of a reset env is cleared: its overlay is that of a fresh context at the same state, while
        # a kept env that has just paid a cost shows the indicator
        tw = nat.Context(robot, n, seed=KEY)
        tw.set_state(*first)
        o_a, o_b = ctxs[0].observe(), tw.observe()
        np.testing.assert_array_equal(o_a, o_b)
        im_a, im_b = ctxs[0].render('track', 32, 32, overlays=True), tw.render('track', 32, 32, overlays=True)
        tw.close()
        np.testing.assert_array_equal(im_a[m], im_b[m], err_msg='cost overlay of a reset env')
        paid = ~m & (outs[0][2] != 0)
        overlay_seen += int((im_a[paid] != im_b[paid]).any(axis=(1, 2, 3)).sum())
        overlay_cleared += int((m & (outs[0][2] != 0)).sum())
      state = first
    if t in twin_reset or t in twin_control:
      assert (t in schedule) == (t in twin_reset)
      tw = nat.Context(robot, n, seed=KEY)
      tw.set_state(*state)
      twins.append([tw, 5])
  assert not twins and resets_checked >= sum(k not in (_m_zeros, _m_events) for k in schedule.values())
  if not doggo:
    assert event_masks >= 3, 'goal- and cost-driven masks must reset something on at least three occasions'
    assert cost_events > 0, 'no cost event in the rollout'
    assert overlay_seen > 0, 'no kept env showed the cost indicator: the overlay check saw nothing'
    assert overlay_cleared > 0, 'no env was reset right after a step that cost it: the cost bytes were not exercised'
  if case == 'point-haul_box':
    assert awake_by_overlap > 0, 'no reset env had its box spawned over an obstacle'
  print(f'{case}: {n} envs x {T} steps, {resets_checked} masked resets; goal-met {met_events}, cost {cost_events}, '
        f'event masks {event_masks}, boxes spawned over an obstacle {awake_by_overlap}, overlays seen {overlay_seen}, cost bytes cleared {overlay_cleared}')
  for dm in masks:
    dm.free()
  for c in ctxs:
    c.close()


def test_haul_box_config_spawns_boxes_over_obstacles():
  """CPU: with HAUL_CONFIG the restatement's later-episode layouts of the ids and nonces the loop test resets put boxes
  over pillars and vases often enough for a few hundred resets to meet some (R.install_awake = the install's flag rule)."""
  from safe_adaptation_gym_amd import _native
  d = _native.task_desc_default(_tid('haul_box'))
  cfg = _cfg(**HAUL_CONFIG)
  gids = ENV_ID0 + np.arange(203)
  prev = {'ctrl_scale': np.ones((203, 12), np.float32), 'bound': np.full(203, 25, np.float32), 'btn_state': np.ones(203, np.int32),
          'catch_timer': np.zeros(203, np.int32), 'catch_cur': np.ones(203, np.float32), 'catch_next': np.full(203, .2, np.float32)}
  rf, ri, st = R.sample('point', d, cfg, gids, EPISODE0 + 1, KEY, False, prev)
  assert not st.any()
  over = (R.install_awake(rf, ri) & (1 << 10)) != 0
  assert over.mean() > 0.05, over.mean()


# ---------------------------------------------------------------------------------------------------------------------
# nonces, ids, shards, failures
# ---------------------------------------------------------------------------------------------------------------------
KEY2 = (KEY & 0xffffffff, KEY >> 32)


def _twin(nat, c, state=None):
  """A fresh context holding the state of `c` (a checkpoint restored with sag_set_state)."""
  tw = nat.Context(c.robot, c.n_envs, seed=KEY)
  tw.set_state(*(state or c.get_state()))
  return tw


@pytest.mark.gpu
def test_nonce_wraps_to_zero_on_a_masked_reset(nat, oracle):
  """Envs at the last 24-bit nonce: a masked device reset gives them nonce 0 and the records the restatement draws at
  nonce 0, and their next step draws its action noise at (env id, episode 0, step 0) - the device's throughput step equals
  its step on the oracle's noise_ep values of that address and, as a control, not on those of the nonce beside it
  (action_noise 0.5, control range widened 4 x: test_throughput_action_noise_vs_oracle)."""
  from test_gpu_parity import _oracle_noise, _rows_off, _state_tol
  n, config = 131, {'action_noise': 0.5}
  c, descs, doe = _make(nat, 'point', [_tid('go_to_goal'), _tid('press_buttons'), _tid('catch_goal')], n, config=config)
  assert c.reset_device(True, episode0=7)[0] == 0
  f, i = c.get_state()
  i[0::3, R.I_EPISODE] = 0xffffff
  i[1::3, R.I_EPISODE] = 0xfffffe
  f[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 2] *= 4
  c.set_state(f, i)
  pre = c.get_state()
  m = np.arange(n) % 2 == 0
  dm = _DevMask(c)
  rc, st, b = c.reset_device(False, d_mask=dm(m))
  assert rc == 0 and not st.any()
  post = c.get_state()
  _expect_reset('point', descs, doe, _cfg(**config), ENV_ID0 + np.arange(n), KEY, pre, post, m)
  wrapped = m & (pre[1][:, R.I_EPISODE] == 0xffffff)
  assert wrapped.sum() > 10 and (post[1][wrapped, R.I_EPISODE] == 0).all()
  _install_twin(nat, 'point', KEY, post[0][m], post[1][m])
  act = np.random.RandomState(8).uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
  c.step(act)
  d_rf = c.get_state()[0]
  tol = _state_tol(nat, 'point')
  beside = post[1].copy()
  beside[:, R.I_EPISODE] = (beside[:, R.I_EPISODE] + 1) & 0xffffff
  tw = _twin(nat, c, post)
  off = {}
  for name, ri_ in (('own address', post[1]), ('nonce beside it', beside)):
    tw.set_state(*post)
    tw.step(act, _oracle_noise(oracle, ri_, 2, key=KEY2), None)
    off[name] = _rows_off(d_rf, tw.get_state()[0], tol)
  assert not off['own address'].any(), f"{off['own address'].sum()} envs off the noise of their own address"
  assert off['nonce beside it'][wrapped].mean() >= 0.25, 'the comparison does not see the noise'
  dm.free(); tw.close(); c.close()


@pytest.mark.gpu
def test_interleaved_replays_and_device_resets_keep_nonces_and_layouts(nat):
  """sag_reset of all envs, sag_reset of some and masked device resets in a random order, a step between calls: an env's
  nonce advances by one per reset of it and never otherwise, a replay restores the layout the env last received - drawn on
  the device or replayed -, `last` distances and install-time awake flags included (the layout store follows the scatter)."""
  n = 101 if HOSTEMU else 1500
  tids = [_tid('haul_box'), _tid('go_to_goal'), _tid('press_buttons'), _tid('push_box')]
  c, descs, doe = _make(nat, 'point', tids, n, config=HAUL_CONFIG)
  assert c.reset_device(True, episode0=0xfffffa)[0] == 0   # (the nonces wrap within the run)
  dm = _DevMask(c)
  Lf, Li = c.get_state()   # host model of the layout store
  assert (Li[:, R.I_AWAKE] != 0).sum() > 0
  rng = np.random.RandomState(12)
  calls = rng.permutation(['all'] * 6 + ['ids'] * 7 + ['mask'] * 7)
  cfg, gids = _cfg(**HAUL_CONFIG), ENV_ID0 + np.arange(n)
  resets = np.zeros(n, np.int64)
  for call in calls:
    f, i = c.get_state()
    c.step(bu.pursuit_actions(f, i, rng, robot='point'))
    pre = c.get_state()
    np.testing.assert_array_equal(pre[1][:, R.I_EPISODE], (0xfffffa + resets) & 0xffffff)
    if call == 'all':
      m = np.ones(n, bool)
      c.reset()
    elif call == 'ids':
      ids = rng.choice(n, size=n // 3, replace=False).astype(np.int32)   # (unsorted)
      m = np.zeros(n, bool); m[ids] = True
      c.reset(ids)
    else:
      m = rng.rand(n) < 0.3
      rc, st, b = c.reset_device(False, d_mask=dm(m))
      assert rc == 0 and not st.any()
    post = c.get_state()
    resets[m] += 1
    if call == 'mask':
      _expect_reset('point', descs, doe, cfg, gids, KEY, pre, post, m)
      Lf[m], Li[m] = post[0][m], post[1][m]
    else:
      Li[m, R.I_EPISODE] = (Li[m, R.I_EPISODE] + 1) & 0xffffff
      np.testing.assert_array_equal(post[0][m], Lf[m], err_msg=f'{call}: floats of the replayed layout')
      np.testing.assert_array_equal(post[1][m], Li[m], err_msg=f'{call}: ints of the replayed layout')
      np.testing.assert_array_equal(post[0][~m], pre[0][~m])
      np.testing.assert_array_equal(post[1][~m], pre[1][~m])
    np.testing.assert_array_equal(post[1][:, R.I_EPISODE], (0xfffffa + resets) & 0xffffff, err_msg=f'nonces after {call}')
  assert resets.min() >= 6, 'every nonce should wrap within the run'
  dm.free(); c.close()


@pytest.mark.gpu
def test_global_ids_up_to_the_last_int32(nat):
  """env_id0 = 2^31 - n with both key words set: the ids reach 0x7fffffff; records of a first and a masked later reset
  equal the restatement, and the envs step."""
  n = 131
  id0 = 2**31 - n
  c, descs, doe = _make(nat, 'point', [_tid('go_to_goal'), _tid('push_box'), _tid('collect')], n, env_id0=id0)
  gids, cfg = id0 + np.arange(n, dtype=np.int64), _cfg()
  rc, st, b = c.reset_device(True, episode0=0xfffffe)
  assert rc == 0 and not st.any()
  pre = c.get_state()
  rf, ri, _ = _ref_batch('point', descs, doe, cfg, gids, np.full(n, 0xfffffe), KEY, True)
  _assert_records(*pre, rf, ri, maxulp=1)
  assert pre[1][-1, R.I_ENV_ID] == 0x7fffffff
  m = np.arange(n) % 3 != 1
  dm = _DevMask(c)
  rc, st, b = c.reset_device(False, d_mask=dm(m))
  assert rc == 0 and not st.any()
  post = c.get_state()
  _expect_reset('point', descs, doe, cfg, gids, KEY, pre, post, m)
  _install_twin(nat, 'point', KEY, post[0][m], post[1][m])
  tw = _twin(nat, c, post)
  act = np.random.RandomState(1).uniform(-1, 1, (n, 2)).astype(np.float32)
  for _ in range(3):
    _same(c.step(act)[:5], tw.step(act)[:5], 'outputs of the checkpoint twin')
  _same(c.get_state(), tw.get_state(), 'state of the checkpoint twin')
  dm.free(); tw.close(); c.close()


def _serial(env):
  """The host emulation of the device sources runs one kernel at a time: the shards of an env take turns there."""
  if HOSTEMU and env._pool is not None:
    env._pool.shutdown()
    env._pool = None
  return env


def _make_env(robot, task, **kw):
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import benchmark
  env = _serial(sag.make(robot, None, device_reset=True, **kw))
  env.set_task(benchmark.TASKS[task])
  return env


def _np(x):
  if isinstance(x, list):
    return np.concatenate([_np(v) for v in x])
  return x.numpy() if hasattr(x, 'numpy') else np.asarray(x)


@pytest.mark.gpu
@pytest.mark.parametrize('robot,task', [('point', 'go_to_goal'), ('car', 'push_box')])
def test_sharded_env_masked_resets_equal_one_context(nat, robot, task):
  """make(..., device_reset=True, devices=[0, 0, 0]) beside one context: host masks that leave one shard's slice empty
  and fill another's; state and the returned observation identical after every reset(mask) and every step."""
  n = 130 if HOSTEMU else 1000
  one = _make_env(robot, task, n_envs=n, seed=17)
  three = _make_env(robot, task, n_envs=n, seed=17, devices=[0, 0, 0])
  (s0, e0), (s1, e1), (s2, e2) = three._ranges
  np.testing.assert_array_equal(one.reset(), three.reset())
  _same(one.get_state(), three.get_state(), 'state after reset()')
  rng = np.random.RandomState(2)
  for cycle in range(3):
    for _ in range(4):
      f, i = one.get_state()
      act = bu.pursuit_actions(f, i, rng, robot=robot)
      a, b = one.step(act), three.step(act)
      _same([a[0], a[1], a[2], a[3]['cost'], a[3]['goal_met'], a[3]['bound']],
            [b[0], b[1], b[2], b[3]['cost'], b[3]['goal_met'], b[3]['bound']], f'cycle {cycle}: step')
      _same(one.get_state(), three.get_state(), f'cycle {cycle}: state after a step')
    m = rng.rand(n) < 0.3
    empty, full = [(s0, e0), (s1, e1), (s2, e2)][cycle], [(s1, e1), (s2, e2), (s0, e0)][cycle]
    m[empty[0]:empty[1]] = False
    m[full[0]:full[1]] = True
    mask = m if cycle != 1 else m.astype(np.uint8) * 3
    pre = one.get_state()
    np.testing.assert_array_equal(one.reset(mask=mask), three.reset(mask=mask), err_msg=f'cycle {cycle}: observation of reset(mask)')
    post = one.get_state()
    _same(post, three.get_state(), f'cycle {cycle}: state after reset(mask)')
    _expect_reset(robot, one._descs, one._desc_of_env, _cfg(), np.arange(n), one._base_seed, pre, post, m)
  one.close(); three.close()


@pytest.mark.gpu
def test_partial_failure_installs_nothing(nat):
  """Two descriptors, one of which cannot be laid out (its extents are smaller than the keep-outs of its items): a mask over
  feasible envs succeeds; a mask with one impossible env returns the failure count, -1 at exactly that env, and leaves the
  state, the nonces and the layout store as they were - the next step equals that of a checkpoint taken before the call."""
  n = 67
  good = nat.task_desc_default(_tid('go_to_goal'))
  bad = dict(good, extents=[-0.5, -0.5, 0.5, 0.5])   # robot within +-0.1, every hazard within +-0.3: never 0.6 apart
  impossible = np.array([5, 40, n - 1])
  doe = np.zeros(n, np.int32)
  c = nat.Context('point', n, seed=KEY)
  c.set_tasks([good, bad], doe, None, env_id0=ENV_ID0)
  assert c.reset_device(True, episode0=3)[0] == 0
  layout = c.get_state()
  doe[impossible] = 1
  c.set_tasks([good, bad], doe, None, env_id0=ENV_ID0)
  descs, cfg, gids = [good, bad], _cfg(), ENV_ID0 + np.arange(n)
  dm = _DevMask(c)
  rng = np.random.RandomState(4)
  act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
  for _ in range(3):
    c.step(act)
  c.reset(); layout[1][:, R.I_EPISODE] += 1
  _same(layout, c.get_state(), 'the replayed layout')
  layout_f, layout_i = layout[0].copy(), layout[1].copy()
  c.step(act)
  # feasible envs only
  m = rng.rand(n) < 0.4
  m[impossible] = False
  pre = c.get_state()
  rc, st, b = c.reset_device(False, d_mask=dm(m))
  assert rc == 0 and not st.any()
  post = c.get_state()
  _expect_reset('point', descs, doe, cfg, gids, KEY, pre, post, m)
  layout_f[m], layout_i[m] = post[0][m], post[1][m]
  c.step(act)
  # one impossible env among feasible ones
  m = rng.rand(n) < 0.4
  m[impossible] = False
  m[impossible[1]] = True
  pre = c.get_state()
  tw = _twin(nat, c, pre)
  rc, st, b = c.reset_device(False, d_mask=dm(m))
  want = np.zeros(n, np.int32); want[impossible[1]] = -1
  assert rc == 1
  np.testing.assert_array_equal(st, want)
  np.testing.assert_array_equal(b, pre[0][:, R.F_BOUND])
  _same(pre, c.get_state(), 'state after a failed reset')
  _same(c.step(act)[:5], tw.step(act)[:5], 'step after a failed reset')
  _same(c.get_state(), tw.get_state(), 'state one step after a failed reset')
  c.reset()   # the layout store: what every env last received
  layout_i[:, R.I_EPISODE] += 1
  _same((layout_f, layout_i), c.get_state(), 'layout store after a failed reset')
  dm.free(); tw.close(); c.close()


@pytest.mark.gpu
def test_a_million_envs_split_equals_single_across_masked_resets(nat, monkeypatch):
  """The size at which early_fork and thousands of busy wavefronts are live: 1 M Point / go_to_goal envs, 10 steps, a masked
  device reset every 3 steps (done | goal_met plus a random 5 %), split against single launch bit for bit."""
  if HOSTEMU:
    pytest.skip('1 M envs: a GPU-sized case (the host emulator runs the same loop at 203 envs)')
  n = 1 << 20
  ctxs, descs, doe = _contexts(nat, monkeypatch, [{'SAG_SPLIT': '0'}, {'SAG_SPLIT': '1'}], 'point', [_tid('go_to_goal')], n, None)
  masks = [_DevMask(c) for c in ctxs]
  for c in ctxs:
    assert c.reset_device(True, episode0=1, want_status=False, want_bound=False)[0] == 0
  rng = np.random.RandomState(6)
  state = ctxs[0].get_state()
  n_reset = 0
  for t in range(10):
    act = bu.pursuit_actions(*state, rng, robot='point')
    outs = [c.step(act) for c in ctxs]
    _same(outs[0][:5], outs[1][:5], f'step {t}: outputs')
    if t % 3 == 2:
      m = (outs[0][3] != 0) | (outs[0][4] != 0) | (rng.rand(n) < 0.05)
      n_reset += int(m.sum())
      for c, dm in zip(ctxs, masks):
        assert c.reset_device(False, d_mask=dm(m), want_bound=False)[0] == 0
    state = ctxs[0].get_state()
    _same(state, ctxs[1].get_state(), f'step {t}: state')
  assert n_reset > 3 * 0.04 * n
  assert ctxs[1].busy_count() > 0
  for dm in masks:
    dm.free()
  for c in ctxs:
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# the env API as documented
# ---------------------------------------------------------------------------------------------------------------------
ROBOT_OBS = {'point': (0, 60), 'car': (1, 72), 'doggo': (2, 104)}


@pytest.mark.gpu
@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
@pytest.mark.parametrize('device_buffers', [False, True])
def test_env_api_masked_reset_cycles(nat, oracle, robot, device_buffers):
  """reset(), then 3 cycles of steps and reset(mask=...): the mask is step()'s own goal_met / done device view
  (device_buffers), a host bool array, a host uint8 array.  Kept rows of the returned observation are the last step's bit
  for bit, reset rows are the oracle's observation of the new state; the state follows the restatement; info['bound']
  (random_bound) stays each env's own across the reset."""
  from test_gpu_parity import OBS_TOL
  n = (70 if robot == 'doggo' else 130) if HOSTEMU else 1000
  rid, od = ROBOT_OBS[robot]
  nu = 12 if robot == 'doggo' else 2
  config = {'random_bound': 1}
  env = _make_env(robot, 'go_to_goal', n_envs=n, seed=23, device_buffers=device_buffers, config=config)
  cfg = _cfg(**config)
  obs = _np(env.reset())
  f, i = env.get_state()
  np.testing.assert_allclose(obs, oracle.observe_batch(oracle.make_batch(f, i), rid, od), rtol=0, atol=OBS_TOL)
  bound = f[:, R.F_BOUND].copy()
  assert len(np.unique(bound)) > n // 2
  rng = np.random.RandomState(9)
  kinds = ['met view', 'done view', 'host uint8'] if device_buffers else ['host bool', 'host uint8', 'host bool']
  n_reset = 0
  for cycle, kind in enumerate(kinds):
    for k in range(3):
      if k == 2:   # goals onto a quarter of the robots: the last step of the cycle meets them
        f, i = env.get_state()
        g = rng.rand(n) < 0.25
        f[g, nat.F_GOAL:nat.F_GOAL + 2] = f[g, nat.F_ROBOT:nat.F_ROBOT + 2]
        env.set_state(f, i)
      act = rng.uniform(-1, 1, (n, nu)).astype(np.float32)
      if robot == 'doggo' and cycle == 0:
        act[:] = 0
      out = env.step(act)
      np.testing.assert_array_equal(out[3]['bound'], bound)
    last_obs, met, done = _np(out[0]).copy(), _np(out[3]['goal_met']) != 0, _np(out[2]) != 0
    if kind == 'met view':
      mask, m = out[3]['goal_met'], met
      assert isinstance(mask, nat.DeviceArray)
    elif kind == 'done view':
      mask, m = out[2], done
    elif kind == 'host bool':
      mask = m = met | (rng.rand(n) < 0.1)
    else:
      m = met | (rng.rand(n) < 0.1)
      mask = m.astype(np.uint8) * 201
    if kind != 'done view':
      assert m.sum() > n // 8, 'the mask should select the envs whose goal was met'
    pre = env.get_state()
    obs = _np(env.reset(mask=mask))
    post = env.get_state()
    _expect_reset(robot, env._descs, env._desc_of_env, cfg, np.arange(n), env._base_seed, pre, post, m)
    np.testing.assert_array_equal(obs[~m], last_obs[~m], err_msg=f'{kind}: kept rows of the observation')
    want = oracle.observe_batch(oracle.make_batch(*post), rid, od)
    np.testing.assert_allclose(obs[m], want[m], rtol=0, atol=OBS_TOL, err_msg=f'{kind}: observation of the reset envs')
    np.testing.assert_array_equal(post[0][:, R.F_BOUND], bound)
    np.testing.assert_array_equal(env._bounds, bound)
    n_reset += int(m.sum())
  out = env.step(rng.uniform(-1, 1, (n, nu)).astype(np.float32))
  np.testing.assert_array_equal(out[3]['bound'], bound)
  assert n_reset > n // 4
  env.close()


@pytest.mark.gpu
def test_env_api_masked_reset_with_rgb_observation(nat, oracle):
  """rgb_observation with masked resets (doggo / haul_box, 24 envs): the returned images are the oracle's render of
  get_state() within the pixel budget of test_rgb_observation_matches_oracle (0.1 % of the pixels), and every differing pixel is
  one that the independent reference (tests/render_ref.py) leaves open."""
  n = 24
  env = _make_env('doggo', 'haul_box', n_envs=n, seed=31, rgb_observation=True)
  env.reset()
  rng = np.random.RandomState(1)
  for cycle in range(2):
    for _ in range(3):
      env.step(rng.uniform(-1, 1, (n, 12)).astype(np.float32))
    pre = env.get_state()
    m = np.arange(n) % 3 == cycle
    img = env.reset(mask=m)
    assert img.shape == (n, 64, 64, 3) and img.dtype == np.uint8
    f, i = env.get_state()
    np.testing.assert_array_equal(f[~m], pre[0][~m])
    assert (f[m, R.F_ROBOT] != pre[0][m, R.F_ROBOT]).all()
    ref = np.stack([oracle.render_rgb(oracle.env(f[k], i[k]), 2) for k in range(n)])
    bad = np.abs(img.astype(int) - ref.astype(int)).max(-1) > 0
    assert bad.mean() <= 1e-3, f'{bad.sum()} pixels differ'
    assert bad[m].mean() <= 1e-3, f'{bad[m].sum()} pixels of the reset envs differ'
    rr.differing_pixels(oracle, img, ref, f, i, 2, 0, 64, 64, what=f'test_env_api_masked_reset_with_rgb_observation cycle {cycle}')
  env.close()


@pytest.mark.gpu
def test_env_api_mask_errors(nat):
  """What reset(mask=...) refuses, each with ValueError and before anything is reset."""
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import benchmark
  n = 40
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True)
  env.reset()
  out = env.step(np.zeros((n, 2), np.float32))
  before = env.get_state()
  c = env._ctx[0]
  p = c.dev_alloc(4 * n)
  bad = [np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n - 1, bool), np.zeros((n, 1), np.uint8),
         nat.DeviceArray(c, p.value, (n,), np.float32), nat.DeviceArray(c, p.value, (n - 1,), np.uint8),
         nat.DeviceArray(c, p.value, (n,), np.uint8, strides=(2,)), out[0]]
  for mask in bad:
    with pytest.raises(ValueError):
      env.reset(mask=mask)
  with pytest.raises(ValueError):
    env.reset(mask=np.ones(n, bool), options={'task': benchmark.TASKS['go_to_goal']})
  _same(before, env.get_state(), 'state after refused masks')
  c.dev_free(p)
  env.close()
  two = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True, devices=[0, 0])
  two.reset()
  out = two.step(np.zeros((n, 2), np.float32))
  with pytest.raises(ValueError):
    two.reset(mask=out[3]['goal_met'][0])   # one device mask for two shards
  two.reset(mask=out[3]['goal_met'])        # (one per shard is the form)
  two.close()
  plain = _serial(sag.make('point', 'go_to_goal', n_envs=n, seed=5))
  plain.reset()
  with pytest.raises(ValueError):
    plain.reset(mask=np.ones(n, bool))      # mask without device_reset
  plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# lockstep against both oracle builds across masked device resets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle32():
  from oracle_lib import Oracle
  return Oracle(f32=True)


@pytest.mark.gpu
@pytest.mark.parametrize('robot,task', [('point', 'multitask'), ('car', 'multitask'), ('point', 'haul_box')])
def test_step_lockstep_throughput_across_device_resets(nat, oracle, oracle32, robot, task):
  """test_step_lockstep_throughput_vs_oracle on device-drawn layouts with three masked device resets in the rollout (two
  driven by the goals met and costs paid since the env's episode began, one random 30 %): the device redraws its noise from the new (episode, step 0) address while the
  oracle legs draw theirs from the record, and the first step of every new episode must reproduce reward (from `last`
  recomputed in fp64), goal-met, task ints, words used and cost flags under _lockstep's own rules, tolerances and budgets."""
  from test_gpu_parity import _lockstep
  # (haul_box with HAUL_CONFIG: boxes spawned over pillars and vases are pushed apart in the first steps of the new episodes)
  _lockstep(nat, oracle, oracle32, robot, task, 1, throughput=True, resets={30: 'random', 65: 'events', 100: 'events'},
            config=HAUL_CONFIG if task == 'haul_box' else None)


@pytest.mark.gpu
def test_doggo_lockstep_throughput_across_a_device_reset(nat, oracle):
  """test_doggo_lockstep_throughput_vs_oracle on device-drawn layouts, with one masked device reset (a random 30 %) after
  the robots have landed."""
  from test_gpu_parity import _doggo_lockstep
  _doggo_lockstep(nat, oracle, 'multitask', throughput=True, reset_after=10)

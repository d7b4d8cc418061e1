"""The rollout loop on the context stream: sag_episode_track_device (csrc/sag_rollout.hpp) and the stream-ordered masked
device reset sag_reset_device_async, against the synchronous sag_reset_device - whose sampler, install and following steps
tests/test_device_reset.py and tests/test_reset_loop.py tie to the restatement and the oracle - bit for bit, and the env
switches time_limit / auto_reset / reset(sync=False) against the loop written by hand with today's calls.

Every GPU test here also runs on the sanitizer host build (tests/hostemu/run.sh) at the reduced sizes given first."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import reset_sampler_ref as R
from test_device_reset import KEY, ROOT, _cfg
from test_reset_loop import (CASES, ENV_ID0, EPISODE0, HOSTEMU, _actions, _contexts, _DevMask, _expect_reset, _m_bytes, _m_events,
                             _m_first, _m_last, _m_ones, _m_random, _m_zeros, _make_env, _np, _same, _tid, _twin)

# step -> mask applied after it (a rollout shorter than the schedule applies what falls into it)
SCHEDULE = {3: _m_events, 4: _m_random, 9: _m_zeros, 10: _m_ones, 15: _m_last, 16: _m_first, 21: _m_bytes, 26: _m_events}
SENTINEL = np.float32(-777.25)


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


class _DevStep:
  """The device buffers of one context's sag_step_device, and the step through them."""

  def __init__(self, c):
    n, nu, od = c.n_envs, c.info['nu'], c.info['obs_dim']
    self.c, self.shapes = c, {'act': ((n, nu), np.float32), 'obs': ((n, od), np.float32), 'rew': ((n, 2), np.float32),
                              'cost': ((n,), np.uint8), 'done': ((n,), np.uint8), 'met': ((n,), np.uint8)}
    self.b = {k: c.dev_alloc(int(np.prod(s)) * np.dtype(d).itemsize) for k, (s, d) in self.shapes.items()}

  def enqueue(self, act):
    b = self.b
    self.c.dev_upload(b['act'], np.ascontiguousarray(act, np.float32))
    self.c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])

  def get(self, k):
    return self.c.dev_download(self.b[k], *self.shapes[k])

  def outputs(self):
    self.c.wait()
    return [self.get(k) for k in ('obs', 'rew', 'cost', 'done', 'met')]

  def step(self, act):
    self.enqueue(act)
    return self.outputs()

  def free(self):
    for p in self.b.values():
      self.c.dev_free(p)


GOAL_TASKS = ('go_to_goal', 'go_to_goal_damping', 'go_to_goal_motor', 'go_to_goal_scarce', 'catch_goal')


def _goals_onto_robots(nat, ctxs, rng):
  """The goals of a quarter of the envs onto their robots (test_env_api_masked_reset_cycles): the next step meets them.
  In a mixed batch only some tasks are met by the robot reaching the goal position (the others press buttons or move an
  object), so the quarter is drawn from the envs of those tasks first and filled up from the rest."""
  f, i = ctxs[0].get_state()
  n = len(f)
  reach = np.isin(i[:, R.I_TASK], [_tid(t) for t in GOAL_TASKS])
  order = rng.permutation(n)
  g = order[np.argsort(~reach[order], kind='stable')][:n // 4]
  f[g, nat.F_GOAL:nat.F_GOAL + 2] = f[g, nat.F_ROBOT:nat.F_ROBOT + 2]
  for c in ctxs:
    c.set_state(f, i)
  return f, i


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['point-mixed', 'car-mixed', 'doggo-mixed'])
def test_async_reset_equals_synchronous_reset(nat, monkeypatch, case):
  """A: sag_reset_device with a mask.  B: sag_reset_device_async with the same mask and the observation buffer its step
  filled.  C (Point, Car): the same under SAG_SPLIT=0, the all-ones mask given as NULL.  State after every reset and every
  step, the five outputs, the busy counts of the split form (stale hot records would show there), the rows of the
  observation buffer inside (= A.observe()) and outside the mask (= what the step wrote) and the counters."""
  robot, pick, config = CASES[case]
  doggo = robot == 'doggo'
  n = (70 if HOSTEMU else 300) if doggo else (203 if HOSTEMU else 1500)
  assert n % 64 and n % 256
  T = 17 if doggo else 30
  tids, doe = pick(n)
  forms = [{}, {}] if doggo else [{'SAG_SPLIT': '1'}, {'SAG_SPLIT': '1'}, {'SAG_SPLIT': '0'}]
  ctxs, descs, doe = _contexts(nat, monkeypatch, forms, robot, tids, n, doe, config=config)
  A, others = ctxs[0], ctxs[1:]
  for c in ctxs:
    rc, st, b = c.reset_device(True, episode0=EPISODE0)
    assert rc == 0 and not st.any()
  devs = [_DevStep(c) for c in others]
  masks = [_DevMask(c) for c in ctxs]
  rng = np.random.RandomState(5)
  state = A.get_state()
  total = 0
  for t in range(T):
    if SCHEDULE.get(t) is _m_events:
      state = _goals_onto_robots(nat, ctxs, rng)
    act = _actions(robot, *state, rng, t)
    out = A.step(act)[:5]
    state = A.get_state()
    for k, d in enumerate(devs, 1):
      _same(out, d.step(act), f'step {t}: outputs of context {k}')
      _same(state, d.c.get_state(), f'step {t}: state of context {k}')
    if not doggo:
      assert others[0].busy_count() == A.busy_count(), f'step {t}: busy envs of the split form'
    if t not in SCHEDULE:
      continue
    kind = SCHEDULE[t]
    m8 = kind(n, rng, out)
    m = m8 != 0
    print(f'{case}: mask after step {t}: {int(m.sum())} of {n} envs')
    if kind is _m_events:
      assert m.sum() > n // 8, 'the events mask should select the envs whose goal was met'
    total += int(m.sum())
    rc, st, b = A.reset_device(False, d_mask=masks[0](m8))
    assert rc == 0 and not st.any()
    state = A.get_state()
    want = A.observe()
    for k, (d, dm) in enumerate(zip(devs, masks[1:]), 1):
      null = kind is _m_ones and k == 2
      d.c.reset_device_async(None if null else dm(m8), d.b['obs'])
      d.c.wait()
      _same(state, d.c.get_state(), f'reset after step {t}: state of context {k}')
      obs = d.get('obs')
      np.testing.assert_array_equal(obs[~m], out[0][~m], err_msg=f'reset after step {t}: a row outside the mask was written')
      np.testing.assert_array_equal(obs[m], want[m], err_msg=f'reset after step {t}: observation of the reset envs')
  for d in devs:
    assert d.c.reset_counts() == (total, 0)
    assert d.c.reset_counts(clear=True) == (total, 0) and d.c.reset_counts() == (0, 0)
    d.free()
  for dm in masks:
    dm.free()
  for c in ctxs:
    c.close()


@pytest.mark.gpu
def test_async_reset_takes_the_steps_flags_without_a_host_wait(nat, monkeypatch):
  """step -> reset(mask = that step's goal_met buffer, obs = its obs buffer) -> step, enqueued back to back and joined once,
  against the same through the synchronous calls."""
  n = 130 if HOSTEMU else 1000
  (A, B), descs, doe = _contexts(nat, monkeypatch, [{}, {}], 'point', [_tid('go_to_goal')], n, None)
  for c in (A, B):
    assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  d, dm = _DevStep(B), _DevMask(A)
  rng = np.random.RandomState(11)
  n_reset = 0
  for cycle in range(3):
    _goals_onto_robots(nat, (A, B), rng)
    a1, a2 = (rng.uniform(-1, 1, (n, 2)).astype(np.float32) for _ in range(2))
    d.enqueue(a1)
    B.reset_device_async(d.b['met'], d.b['obs'])
    d.enqueue(a2)
    out_b = d.outputs()
    met = A.step(a1)[4]
    assert met.sum() > n // 8
    n_reset += int(met.sum())
    assert A.reset_device(False, d_mask=dm(met))[0] == 0
    _same(A.step(a2)[:5], out_b, f'cycle {cycle}: outputs of the second step')
    _same(A.get_state(), B.get_state(), f'cycle {cycle}: state')
  assert B.reset_counts() == (n_reset, 0)
  d.free(); dm.free(); A.close(); B.close()


@pytest.mark.gpu
def test_async_reset_commits_env_by_env(nat):
  """The scenario of test_partial_failure_installs_nothing through the stream-ordered call: the feasible envs of the mask
  are reset, the impossible one keeps state, nonce, observation row and layout-store row and gets the ResamplingError bit."""
  n = 67
  good = nat.task_desc_default(_tid('go_to_goal'))
  bad = dict(good, extents=[-0.5, -0.5, 0.5, 0.5])   # robot within +-0.1, every hazard within +-0.3: never 0.6 apart
  imp = 40
  doe = np.zeros(n, np.int32)
  c = nat.Context('point', n, seed=KEY)
  c.set_tasks([good, bad], doe, None, env_id0=ENV_ID0)
  assert c.reset_device(True, episode0=3)[0] == 0
  layout_f, layout_i = c.get_state()
  doe[imp] = 1
  c.set_tasks([good, bad], doe, None, env_id0=ENV_ID0)
  descs, cfg, gids = [good, bad], _cfg(), ENV_ID0 + np.arange(n)
  d, dm = _DevStep(c), _DevMask(c)
  rng = np.random.RandomState(4)
  act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
  for _ in range(3):
    out = d.step(act)
  m = rng.rand(n) < 0.4
  m[imp] = True
  feasible = m.copy(); feasible[imp] = False
  pre = c.get_state()
  c.reset_device_async(dm(m), d.b['obs'])
  c.wait()
  post = c.get_state()
  assert c.reset_counts() == (int(feasible.sum()), 1)
  assert post[1][imp, R.I_FLAGS] == pre[1][imp, R.I_FLAGS] | 1 and not pre[1][imp, R.I_FLAGS] & 1
  np.testing.assert_array_equal(post[1][imp, R.I_EPISODE], pre[1][imp, R.I_EPISODE])
  unflagged = (post[0], post[1].copy())
  unflagged[1][imp, R.I_FLAGS] = pre[1][imp, R.I_FLAGS]
  _expect_reset('point', descs, doe, cfg, gids, KEY, pre, unflagged, feasible)
  obs = d.get('obs')
  np.testing.assert_array_equal(obs[~feasible], out[0][~feasible], err_msg='rows of the kept envs and of the impossible one')
  np.testing.assert_array_equal(obs[feasible], c.observe()[feasible])
  tw = _twin(nat, c, post)
  _same(d.step(act), tw.step(act)[:5], 'step after the reset')
  _same(c.get_state(), tw.get_state(), 'state one step after the reset')
  c.reset()   # the layout store: what every env last received
  layout_f[feasible], layout_i[feasible] = post[0][feasible], post[1][feasible]
  layout_i[:, R.I_EPISODE] = np.where(feasible, post[1][:, R.I_EPISODE], pre[1][:, R.I_EPISODE]) + 1
  _same((layout_f, layout_i), c.get_state(), 'layout store after the reset')
  d.free(); dm.free(); tw.close(); c.close()


def _track_ref(acc, rew, cost, done, met, max_steps, episode):
  """NumPy restatement of k_episode_track: float32 adds in the order of the calls."""
  acc[:, 0] = acc[:, 0] + rew[:, 0]
  acc[:, 1] += cost != 0
  acc[:, 2] += 1
  acc[:, 3] += met != 0
  ended = np.where(done != 0, 1, np.where((acc[:, 2] >= max_steps) & (max_steps > 0), 2, 0)).astype(np.uint8)
  e = ended != 0
  episode[e] = acc[e]
  acc[e] = 0
  return ended


@pytest.mark.gpu
@pytest.mark.parametrize('max_steps', [7, 0])
def test_episode_tracker_equals_numpy(nat, max_steps):
  n = 131
  c = nat.Context('point', n, seed=KEY)
  shapes = {'rew': ((n, 2), np.float32), 'cost': ((n,), np.uint8), 'done': ((n,), np.uint8), 'met': ((n,), np.uint8),
            'ended': ((n,), np.uint8), 'episode': ((n, 4), np.float32), 'mask': ((n,), np.uint8)}
  b = {k: c.dev_alloc(int(np.prod(s)) * np.dtype(d).itemsize) for k, (s, d) in shapes.items()}
  get = lambda k: c.dev_download(b[k], *shapes[k])   # noqa: E731
  rng = np.random.RandomState(21)
  acc, episode = np.zeros((n, 4), np.float32), np.full((n, 4), SENTINEL, np.float32)
  c.dev_upload(b['episode'], episode)
  ever = np.zeros(n, bool)

  def call(rew, cost, done, met, ms, what):
    for k, v in (('rew', rew), ('cost', cost), ('done', done), ('met', met)):
      c.dev_upload(b[k], v)
    c.episode_track(b['rew'], b['cost'], b['done'], b['met'], ms, b['ended'], b['episode'])
    c.wait()
    ended = _track_ref(acc, rew, cost, done, met, ms, episode)
    np.testing.assert_array_equal(get('ended'), ended, err_msg=f'{what}: ended')
    np.testing.assert_array_equal(get('episode'), episode, err_msg=f'{what}: episode rows')
    return ended

  def draw():
    rew = rng.randn(n, 2).astype(np.float32)
    return rew, (rng.rand(n) < 0.2).astype(np.uint8), (rng.rand(n) < 0.05).astype(np.uint8) * 3, (rng.rand(n) < 0.2).astype(np.uint8)

  seen = set()
  for k in range(40):
    ended = call(*draw(), max_steps, f'call {k}')
    ever |= ended != 0
    seen |= set(ended.tolist())
    if k == 19:
      m = (rng.rand(n) < 0.3).astype(np.uint8)
      c.dev_upload(b['mask'], m)
      c.episode_clear(b['mask'])
      acc[m != 0] = 0
  assert seen == ({0, 1, 2} if max_steps else {0, 1})
  if not max_steps:
    assert (~ever).sum() > 0 and (episode[~ever] == SENTINEL).all(), 'rows of envs that never ended hold the sentinel'
  assert (acc[:, 2] > 0).any() and (acc[:, 0] != 0).any()
  # the accumulators themselves: a call that ends every episode writes them out
  rew, cost, done, met = draw()
  call(rew, cost, np.ones(n, np.uint8), met, max_steps, 'flush')
  assert not acc.any()
  for k in range(3):
    call(*draw(), 0, f'refill {k}')
  c.episode_clear()
  acc[:] = 0
  rew, cost, done, met = draw()
  call(rew, cost, np.ones(n, np.uint8), met, max_steps, 'after a clear of every env')
  np.testing.assert_array_equal(episode[:, 2], 1)
  for p in b.values():
    c.dev_free(p)
  c.close()


@pytest.mark.gpu
@pytest.mark.parametrize('devices', [None, [0, 0, 0]], ids=['1 shard', 'devices=[0, 0, 0]'])
def test_env_auto_reset_equals_manual_loop(nat, devices):
  """make(..., time_limit=5, auto_reset=True), stepped with sync=False, beside an env without the switches that keeps a NumPy
  tracker on the host and calls today's reset(mask=ended) after every step."""
  n, limit = (130 if HOSTEMU else 1000), 5
  kw = {} if devices is None else {'devices': devices}
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=29, device_buffers=True, time_limit=limit, auto_reset=True, **kw)
  twin = _make_env('point', 'go_to_goal', n_envs=n, seed=29)
  np.testing.assert_array_equal(_np(env.reset()), twin.reset())
  _same(env.get_state(), twin.get_state(), 'state after reset()')
  rng = np.random.RandomState(13)
  acc, episode = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
  m30 = rng.rand(n) < 0.3
  expect = {5: ~m30, 8: m30, 10: ~m30, 13: m30, 15: ~m30}
  n_reset = 0
  for k in range(1, 18):
    act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    obs, rew, done, info = env.step(act, sync=False)
    env.wait()
    t_obs, t_rew, t_done, t_info = twin.step(act)
    ended = _track_ref(acc, np.stack([t_rew, t_rew], 1), t_info['cost'], t_done, t_info['goal_met'], limit, episode)
    t_obs = twin.reset(mask=ended)
    n_reset += int((ended != 0).sum())
    e = ended != 0
    _same([_np(obs), _np(rew), _np(done), _np(info['terminated']) != 0, _np(info['cost']) != 0, _np(info['goal_met']) != 0, info['bound']],
          [t_obs, t_rew, ended, t_done, t_info['cost'] != 0, t_info['goal_met'], t_info['bound']], f'step {k}')
    np.testing.assert_array_equal(_np(info['episode'])[e], episode[e], err_msg=f'step {k}: episode rows of the ended envs')
    _same(env.get_state(), twin.get_state(), f'step {k}: state')
    np.testing.assert_array_equal(ended == 2, expect.get(k, np.zeros(n, bool)) & (t_done == 0), err_msg=f'step {k}: truncated envs')
    if k == 3:
      obs = env.reset(mask=m30, sync=False)
      env.wait()
      np.testing.assert_array_equal(_np(obs), twin.reset(mask=m30), err_msg='observation of reset(mask, sync=False)')
      _same(env.get_state(), twin.get_state(), 'state after reset(mask, sync=False)')
      acc[m30] = 0
      n_reset += int(m30.sum())
  assert env.reset_counts() == (n_reset, 0)
  env.close(); twin.close()


@pytest.mark.gpu
def test_env_api_refusals(nat):
  """What the new switches refuse, each with ValueError: at construction, or at the call before anything is enqueued."""
  import safe_adaptation_gym_amd as sag
  n = 40
  for kw in ({'time_limit': 5}, {'auto_reset': True}, {'time_limit': 5, 'auto_reset': True}):
    for base in ({}, {'device_buffers': True}, {'device_reset': True}, {'device_buffers': True, 'device_reset': True, 'parity_rng': True},
                 {'parity_rng': True}, {'device_buffers': True, 'device_reset': True, 'rgb_observation': True}):
      with pytest.raises(ValueError):
        sag.make('point', 'go_to_goal', n_envs=n, seed=5, **base, **kw)
  with pytest.raises(ValueError):
    sag.make('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True, device_reset=True, time_limit=0)
  for base in ({'device_reset': True}, {'device_buffers': True}, {}):
    env = _make_env('point', 'go_to_goal', n_envs=n, seed=5) if base.get('device_reset') else sag.make(
        'point', 'go_to_goal', n_envs=n, seed=5, **base)
    env.reset()
    env.step(np.zeros((n, 2), np.float32))
    before = env.get_state()
    for mask in (None, np.ones(n, bool)) if base.get('device_reset') else (None,):
      with pytest.raises(ValueError):
        env.reset(mask=mask, sync=False)
    _same(before, env.get_state(), f'state after a refused reset(sync=False) of {base}')
    env.close()
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True, time_limit=5)
  env.reset()
  env.step(np.zeros((n, 2), np.float32))
  before = env.get_state()
  for mask in (np.zeros(n, np.float32), np.zeros(n - 1, bool)):
    with pytest.raises(ValueError):
      env.reset(mask=mask, sync=False)
  _same(before, env.get_state(), 'state after refused masks')
  assert env.reset_counts() == (0, 0)
  env.close()


def test_async_reset_cases_on_the_sanitizer_build():
  """This file's GPU cases (without the Doggo: tests/hostemu/run.sh runs it) on the ASan / UBSan host build of the library's
  sources, as test_device_reset.test_masked_reset_kernels_on_the_sanitizer_build: no report, every case passed, none skipped."""
  sys.path.insert(0, os.path.join(ROOT, 'tests', 'hostemu'))
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.fail('no clang for the host build of the kernel')
  lib = hb.build('clang', False, True, [], False, False, 'san')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'),
             ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:detect_stack_use_after_return=0:halt_on_error=1',
             UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
  env['LD_PRELOAD'] = os.pathsep.join([hb.preload('clang')] + ([os.environ['LD_PRELOAD']] if os.environ.get('LD_PRELOAD') else []))
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-k', 'not doggo', '-q', '-p', 'no:cacheprovider'],
                     env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
  tail = r.stdout[-3000:] + r.stderr[-3000:]
  assert r.returncode == 0, tail
  assert 'Sanitizer' not in r.stdout + r.stderr and 'runtime error' not in r.stdout + r.stderr, tail
  summary = r.stdout.strip().splitlines()[-1]
  passed = re.search(r'(\d+) passed', summary)
  assert passed and int(passed.group(1)) == 9 and 'skipped' not in summary and 'failed' not in summary, summary

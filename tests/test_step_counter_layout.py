"""Where the step counter lives on the device (csrc/sag_device.hpp: DF_STEP, DI_PSZ).  SAG_I_STEP travels as int32 bits in
the last float of group 1, which every step stores whole; the pillar-size float travels as bits in the int4 word group, which
no step rewrites.  The record (include/sag.h) is unchanged, so everything here goes through the public calls: the counter must
come back exact - small counters are denormal bit patterns as floats - whichever kernel (single launch, quiet, busy, Doggo
post) and whichever copy (group-major state, hot record) carried it, and the pillar size bit for bit.

Point and Car / push_box: 1500 envs in the single launch and in the split form with the early fork forced on; Doggo: 64 envs."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_parity import nat  # noqa: F401 (fixture)
from test_reset_loop import _DevMask, _make, _make_env, _np, _tid
from test_state_layout import CAR_BOUND, POINT_BOUND, _place

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batch_util as bu  # noqa: E402
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE, SPLIT = {'SAG_SPLIT': '0', 'SAG_EARLY_FORK': '0'}, {'SAG_SPLIT': '1', 'SAG_EARLY_FORK': '1'}
CASES = {'point': ('point', 'go_to_goal', 1500, (SINGLE, SPLIT)), 'car': ('car', 'push_box', 1500, (SINGLE, SPLIT)),
         'doggo': ('doggo', 'go_to_goal', 64, ({},))}
# 0 and 1: the smallest denormal patterns; 999; 2^23 and above: normal floats, a NaN pattern among them (0x7fc00001)
COUNTERS = np.array([0, 1, 999, 1 << 23, (1 << 23) + 1, 0x3f800000, 0x7f800000, 0x7fc00001, 2, 0x007fffff], np.int64)


def _counters(n, headroom=0):
  """Distinct counters for n envs: the list above first, then 1000 + 7 i (headroom: steps that will still be added)."""
  c = 1000 + 7 * np.arange(n, dtype=np.int64)
  k = min(n, len(COUNTERS))
  c[:k] = COUNTERS[:k]
  assert len(np.unique(c)) == n and c.max() + headroom < 2**31
  return c.astype(np.int32)


def _pillar_sizes(n):
  p = (0.15 + np.arange(n) / 16384.0).astype(np.float32)
  assert len(np.unique(p)) == n
  return p


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def _forms(nat, monkeypatch, case, seed=4000):
  """One context per launch form of the case, all with the same layout -> (contexts, robot, n)."""
  robot, task, n, forms = CASES[case]
  rf, ri = bu.sample_records_native(robot, task, n, seed=seed)
  ctxs = []
  for env in forms:
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    c = nat.Context(robot, n, seed=77)
    c.set_layout(rf, ri)
    ctxs.append(c)
  for k in SPLIT:
    monkeypatch.delenv(k, raising=False)
  return ctxs, robot, n


def _install(nat, ctxs, n, headroom):
  """Distinct counters and pillar sizes into every context -> the records as installed."""
  rf, ri = ctxs[0].get_state()
  ri[:, nat.I_STEP] = _counters(n, headroom)
  rf[:, nat.F_PILLAR_SIZE] = _pillar_sizes(n)
  for c in ctxs:
    c.set_state(rf, ri)
  return rf, ri


def _fixed(nat):
  """Record ints no step may change: what the meta word holds, the env id, the flags and the episode nonce."""
  return [nat.I_TASK, nat.I_NH, nat.I_NV, nat.I_NP, nat.I_NB, nat.I_BOX_KIND, nat.I_ENV_ID, nat.I_FLAGS, nat.I_EPISODE]


def _check(nat, ctxs, rf0, ri0, k, what):
  """Every context: counter = installed + k, pillar size and the fixed ints as installed; all contexts hold the same state."""
  states = [c.get_state() for c in ctxs]
  for q, (f, i) in enumerate(states):
    np.testing.assert_array_equal(i[:, nat.I_STEP].astype(np.int64), ri0[:, nat.I_STEP].astype(np.int64) + k, err_msg=f'{what}: counter, form {q}')
    np.testing.assert_array_equal(_bits(f[:, nat.F_PILLAR_SIZE]), _bits(rf0[:, nat.F_PILLAR_SIZE]), err_msg=f'{what}: pillar size, form {q}')
    np.testing.assert_array_equal(i[:, _fixed(nat)], ri0[:, _fixed(nat)], err_msg=f'{what}: meta / env id / flags, form {q}')
    np.testing.assert_array_equal(_bits(f), _bits(states[0][0]), err_msg=f'{what}: floats of form {q} against form 0')
    np.testing.assert_array_equal(i, states[0][1], err_msg=f'{what}: ints of form {q} against form 0')
  return states[0]


def _close(ctxs):
  for c in ctxs:
    c.close()


@pytest.mark.parametrize('case', list(CASES))
def test_counter_advances_by_one_per_step(nat, monkeypatch, case):
  """(a) after 1, 2 and 7 steps the counter is the installed value + k in every launch form, and nothing else of the int4 or
  the pillar size has changed."""
  ctxs, robot, n = _forms(nat, monkeypatch, case)
  if robot != 'doggo':   # a third of the robots beside a vase, as in test_state_layout: the split form has a busy list
    _place(nat, SimpleNamespace(ctx=ctxs[0]), POINT_BOUND if robot == 'point' else CAR_BOUND, 0.10 if robot == 'point' else 0.16)
  rf0, ri0 = _install(nat, ctxs, n, headroom=7)
  rng = np.random.RandomState(5)
  nu = ctxs[0].info['nu']
  done, busy = 0, []
  for k in (1, 2, 7):
    while done < k:
      act = rng.uniform(-1, 1, (n, nu)).astype(np.float32)
      outs = [c.step(act) for c in ctxs]
      for o in outs[1:]:
        for a, b in zip(outs[0][:5], o[:5]):
          np.testing.assert_array_equal(a, b, err_msg=f'outputs, step {done + 1}')
      done += 1
      busy.append(ctxs[-1].busy_count())
    _check(nat, ctxs, rf0, ri0, k, f'after {k} steps')
  if len(ctxs) > 1:
    assert any(0 < b < n for b in busy), f'the split form used one launch only: {busy}'
  _close(ctxs)


@pytest.mark.parametrize('case', list(CASES))
def test_round_trip_of_counters_and_pillar_sizes(nat, monkeypatch, case):
  """(b) set_state -> get_state of records with distinct counters (0, 1, 999, >= 2^23, NaN and infinity patterns) and distinct
  pillar sizes is exact, twice over."""
  ctxs, robot, n = _forms(nat, monkeypatch, case)
  rf0, ri0 = _install(nat, ctxs, n, headroom=0)
  assert {0, 1, 999, 1 << 23} <= set(ri0[:, nat.I_STEP].tolist())
  for c in ctxs:
    f, i = c.get_state()
    np.testing.assert_array_equal(_bits(f), _bits(rf0))
    np.testing.assert_array_equal(i, ri0)
    c.set_state(f[::-1], i[::-1], env_ids=np.arange(n)[::-1])   # the same records, env by env in another order
    f2, i2 = c.get_state(env_ids=[n - 1, 0, 3])
    np.testing.assert_array_equal(_bits(f2), _bits(rf0[[n - 1, 0, 3]]))
    np.testing.assert_array_equal(i2, ri0[[n - 1, 0, 3]])
  _close(ctxs)


@pytest.mark.parametrize('robot,forms', [('point', (SINGLE, SPLIT)), ('car', (SINGLE, SPLIT)), ('doggo', ({},))])
def test_masked_device_reset_zeroes_the_masked_counters_only(nat, monkeypatch, robot, forms):
  """(c) sag_reset_device and sag_reset_device_async under a mask: counter 0 for the masked envs, untouched for the others."""
  n = 64 if robot == 'doggo' else 1500
  task = 'push_box' if robot == 'car' else 'go_to_goal'
  for env in forms:
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    c, _, _ = _make(nat, robot, [_tid(task)], n)
    rc, st, _ = c.reset_device(True)
    assert rc == 0 and not st.any()
    rf, ri = c.get_state()
    ri[:, nat.I_STEP] = _counters(n, headroom=4)
    c.set_state(rf, ri)
    act = np.zeros((n, c.info['nu']), np.float32)
    c.step(act)
    dm = _DevMask(c)
    expect = ri[:, nat.I_STEP].astype(np.int64) + 1
    for call, m in (('sync', np.arange(n) % 3 == 0), ('async', np.arange(n) % 3 == 1)):
      if call == 'sync':
        rc, st, _ = c.reset_device(False, d_mask=dm(m))
        assert rc == 0 and not st.any()
      else:
        c.reset_device_async(dm(m))
        assert c.reset_counts() == (int(m.sum()), 0)
      expect[m] = 0
      np.testing.assert_array_equal(c.get_state()[1][:, nat.I_STEP], expect, err_msg=f'{call} reset')
      c.step(act)
      expect += 1
      np.testing.assert_array_equal(c.get_state()[1][:, nat.I_STEP], expect, err_msg=f'step after the {call} reset')
    dm.free()
    c.close()
  for k in SPLIT:
    monkeypatch.delenv(k, raising=False)


def test_time_limit_truncates_at_the_limit(nat):
  """(d) make(time_limit=5, auto_reset=True): an env is truncated at exactly five steps of its episode, the tracker's episode
  length is the host's count, and the device counter is that count (0 again after the reset)."""
  n, limit = 1500, 5
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=29, device_buffers=True, time_limit=limit, auto_reset=True)
  env.reset()
  assert not env.get_state()[1][:, nat.I_STEP].any()
  rng = np.random.RandomState(13)
  length = np.zeros(n, np.int64)
  for k in range(1, 13):
    if k == 3:   # a third of the envs start over: their limit is counted from here
      m = np.arange(n) % 3 == 0
      env.reset(mask=m)
      length[m] = 0
    obs, rew, done, info = env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32), sync=False)
    env.wait()
    length += 1
    ended, term = _np(done), _np(info['terminated']) != 0
    np.testing.assert_array_equal(ended == 2, (length == limit) & ~term, err_msg=f'step {k}: truncated envs')
    np.testing.assert_array_equal(ended == 1, term, err_msg=f'step {k}: terminated envs')
    e = ended != 0
    np.testing.assert_array_equal(_np(info['episode'])[e, 2], length[e], err_msg=f'step {k}: episode lengths')
    length[e] = 0
    np.testing.assert_array_equal(env.get_state()[1][:, nat.I_STEP], length, err_msg=f'step {k}: counters')
  env.close()


@pytest.mark.parametrize('case', list(CASES))
def test_fork_copies_counter_and_pillar_size(nat, monkeypatch, case):
  """(e) sag_fork_device: the targets take counter and pillar size of their sources (and keep their own env id); the next step
  - the copies' first, in the busy kernel from refreshed hot records - adds one."""
  ctxs, robot, n = _forms(nat, monkeypatch, case)
  rf0, ri0 = _install(nat, ctxs, n, headroom=3)
  act = np.zeros((n, ctxs[0].info['nu']), np.float32)
  for c in ctxs:
    c.step(act)
  src = (5 * (np.arange(n) // 5)).astype(np.int32)   # groups of five, leader first
  src[n // 2:] = -1
  m = src >= 0
  want_f, want_i = rf0.copy(), ri0.copy()
  want_i[:, nat.I_STEP] += 1
  want_f[m, nat.F_PILLAR_SIZE], want_i[m, nat.I_STEP] = want_f[src[m], nat.F_PILLAR_SIZE], want_i[src[m], nat.I_STEP]
  for k in (0, 1):
    for q, c in enumerate(ctxs):
      if k == 0:
        p = c.dev_alloc(4 * n)
        c.dev_upload(p, src)
        c.fork_device(p)
        copied, rejected = c.fork_counts()
        assert copied > 0 and rejected == 0
        c.dev_free(p)
      else:
        c.step(act)
      f, i = c.get_state()
      np.testing.assert_array_equal(i[:, nat.I_STEP], want_i[:, nat.I_STEP] + k, err_msg=f'counter, form {q}, {k} steps after the fork')
      np.testing.assert_array_equal(_bits(f[:, nat.F_PILLAR_SIZE]), _bits(want_f[:, nat.F_PILLAR_SIZE]), err_msg=f'pillar size, form {q}')
      np.testing.assert_array_equal(i[:, nat.I_ENV_ID], ri0[:, nat.I_ENV_ID], err_msg=f'env id, form {q}')
  _close(ctxs)


def test_counter_follows_an_env_between_quiet_and_busy(nat, monkeypatch):
  """(f) Point / go_to_goal laid out as in test_state_layout (robots beside vases, on goals, approaching vases): envs go quiet
  -> busy -> quiet, so the counter is carried by the quiet kernel, by the busy kernel from hot records written by either, and
  by the group-major state in turn.  The split form equals the single launch after every step."""
  n, steps = 193, 30
  runs = []
  for split in ('1', '0'):
    monkeypatch.setenv('SAG_SPLIT', split)
    runs.append(bench.DeviceRun('go_to_goal', n, 0, 0, robot='point'))
  for r in runs:
    _place(nat, r, POINT_BOUND, 0.10)
  ctxs = [r.ctx for r in runs]
  rf0, ri0 = _install(nat, ctxs, n, headroom=steps)
  busy = []
  for t in range(steps):
    for r in runs:
      r.step()
    a, b = runs[0].outputs(), runs[1].outputs()
    for name in a:
      np.testing.assert_array_equal(a[name].view(np.uint8), b[name].view(np.uint8), err_msg=f'{name}, step {t + 1}')
    _check(nat, ctxs, rf0, ri0, t + 1, f'step {t + 1}')
    busy.append(ctxs[0].busy_count())
  print('busy per step', busy)
  assert all(0 <= x <= n for x in busy) and any(0 < x < n for x in busy), busy
  assert any(y > x for x, y in zip(busy[1:], busy[2:])), f'no quiet env ever turned busy: {busy}'
  assert any(y < x for x, y in zip(busy, busy[1:])), f'no busy env ever turned quiet: {busy}'
  for r in runs:
    r.close()


@pytest.mark.parametrize('case', list(CASES))
def test_observe_does_not_advance_the_counter(nat, monkeypatch, case):
  """(g) sag_observe, before any step and after one: the whole state, counter included, stays as it is."""
  ctxs, robot, n = _forms(nat, monkeypatch, case)
  rf0, ri0 = _install(nat, ctxs, n, headroom=1)
  for c in ctxs:
    c.observe()
  _check(nat, ctxs, rf0, ri0, 0, 'observe() after set_state')
  act = np.full((n, ctxs[0].info['nu']), 0.25, np.float32)
  for c in ctxs:
    c.step(act)
  before = _check(nat, ctxs, rf0, ri0, 1, 'one step')
  obs = [c.observe() for c in ctxs]
  for c, o in zip(ctxs, obs):
    np.testing.assert_array_equal(_bits(c.observe()), _bits(obs[0]), err_msg='observe() twice, and against form 0')
  after = _check(nat, ctxs, rf0, ri0, 1, 'observe() after a step')
  np.testing.assert_array_equal(_bits(after[0]), _bits(before[0]))
  np.testing.assert_array_equal(after[1], before[1])
  _close(ctxs)

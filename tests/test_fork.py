"""Fork on the device: sag_fork_device (csrc/sag_fork.hpp) and env.fork() against the only way to move one env's state into
another that existed before them - get_state(), permute the rows, set_state() on the host -, bit for bit: the state, the five
outputs of the following steps, the busy counts of the split form (stale hot records show there), the layout store that
sag_reset replays, the episode accumulators, the descriptor index a later device reset samples with, and the identity of the
random streams.  The reference of every comparison is that host path or a context that was never forked, never the new code.

Sizes follow tests/test_async_reset.py: the reduced ones come first and are used on the host build of the device sources."""
import numpy as np
import pytest

import reset_sampler_ref as R
from test_device_reset import KEY, _cfg
from test_reset_loop import (CASES, ENV_ID0, EPISODE0, HOSTEMU, _actions, _contexts, _DevMask, _expect_reset, _make, _make_env, _np,
                             _same, _tid, _twin)
from test_async_reset import _DevStep, _goals_onto_robots, _track_ref

INT32_MAX = 2**31 - 1


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


class _DevSrc:
  """A device buffer of one context that carries host source-index arrays to sag_fork_device."""

  def __init__(self, c):
    self.c, self.p = c, c.dev_alloc(4 * c.n_envs)

  def __call__(self, src):
    src = np.ascontiguousarray(src, np.int32)
    assert src.shape == (self.c.n_envs,)
    self.c.dev_upload(self.p, src)
    return self.p

  def free(self):
    self.c.dev_free(self.p)


def _host_fork(c, src, source=None, same_stream=False):
  """The reference: what the fork does, through the host - get_state(), permute the rows by src, every row's own
  SAG_I_ENV_ID, set_state() of the whole batch."""
  sf, si = (source or c).get_state()
  f, i = c.get_state()
  m = src >= 0
  own = i[:, R.I_ENV_ID].copy()
  f[m], i[m] = sf[src[m]], si[src[m]]
  if not same_stream:
    i[:, R.I_ENV_ID] = own
  c.set_state(f, i)


def _permute_layout(lay, src):
  """The host model of the layout store after a fork: rows by src, own env ids."""
  f, i = lay
  m = src >= 0
  own = i[:, R.I_ENV_ID].copy()
  f[m], i[m] = f[src[m]], i[src[m]]
  i[:, R.I_ENV_ID] = own


def _rule_ok(src, n_src, same):
  """NumPy restatement of the commit rule (include/sag.h)."""
  ok = (src >= 0) & (src < n_src)
  if same:
    j = np.where(ok, src, 0)
    ok &= (j == np.arange(len(src))) | (src[j] < 0) | (src[j] == j)
  return ok


def _patterns(n, rng):
  last5 = np.minimum(5 * (np.arange(n) // 5) + 4, n - 1)
  sources = rng.rand(n) < 0.3
  rnd = np.where(rng.rand(n) < 0.8, rng.choice(np.flatnonzero(sources), size=n), -1)
  rnd[sources] = np.where(rng.rand(int(sources.sum())) < 0.5, np.flatnonzero(sources), -1)
  out = [('all negative', np.full(n, -1)), ('from env 0', np.zeros(n, int)), ('from the last env', np.full(n, n - 1)),
         ('groups of 5, leader first', 5 * (np.arange(n) // 5)), ('groups of 5, leader last', last5), ('random', rnd),
         ('random again', rnd)]
  for what, src in out:
    assert _rule_ok(src, n, True)[src >= 0].all(), what
  return [(what, src.astype(np.int32)) for what, src in out]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['point-mixed', 'car-mixed', 'doggo-mixed'])
def test_fork_equals_the_host_path(nat, monkeypatch, case):
  """A: sag_fork_device inside the batch.  B: the same through get_state / set_state.  Point and Car: a second pair under
  SAG_SPLIT=0.  Seven patterns one after the other with steps between; at the end sag_reset of forked envs against the
  control given the permuted layout."""
  robot, pick, config = CASES[case]
  doggo = robot == 'doggo'
  n = (70 if HOSTEMU else 300) if doggo else (203 if HOSTEMU else 1500)
  assert n % 64 and n % 256   # (ipad padding: the reduced sizes here, and 3 / 130 / 67 envs below)
  tids, doe = pick(n)
  forms = [{}, {}] if doggo else [{'SAG_SPLIT': '1'}, {'SAG_SPLIT': '1'}, {'SAG_SPLIT': '0'}, {'SAG_SPLIT': '0'}]
  ctxs, descs, doe = _contexts(nat, monkeypatch, forms, robot, tids, n, doe, config=config)
  pairs = list(zip(ctxs[0::2], ctxs[1::2]))
  for c in ctxs:
    rc, st, b = c.reset_device(True, episode0=EPISODE0)
    assert rc == 0 and not st.any()
  lay = ctxs[0].get_state()   # host model of the layout store
  devs = [_DevSrc(a) for a, _ in pairs]
  rng = np.random.RandomState(7)
  state = ctxs[0].get_state()
  t = 0

  def steps(k, since_fork):
    nonlocal state, t
    for s in range(k):
      act = _actions(robot, *state, rng, t)
      outs = [c.step(act)[:5] for c in ctxs]
      state = ctxs[0].get_state()
      for q, c in enumerate(ctxs[1:], 1):
        _same(outs[0], outs[q], f'step {t}: outputs of context {q}')
        _same(state, c.get_state(), f'step {t}: state of context {q}')
      if not doggo and (since_fork is None or s >= 1):
        assert pairs[0][0].busy_count() == pairs[0][1].busy_count(), f'step {t}: busy envs of the split form'
      t += 1

  steps(3 if doggo else 6, None)
  state = _goals_onto_robots(nat, ctxs, rng)
  # no robot uses the last four floats of the record (the last float4 group of the device state): they carry a tag per env
  state[0][:, -4:] = rng.rand(n, 4)
  for c in ctxs:
    c.set_state(*state)
  steps(2 if doggo else 4, None)
  assert len(np.unique(ctxs[0].get_state()[0][:, -1])) == n
  for what, src in _patterns(n, rng):
    if what == 'random':
      state = _goals_onto_robots(nat, ctxs, rng)
      steps(1, None)
    pre = state
    for (a, b), d in zip(pairs, devs):
      a.fork_device(d(src))
      _host_fork(b, src)
      assert a.fork_counts(clear=True) == (int((src >= 0).sum()), 0), what
    _permute_layout(lay, src)
    state = ctxs[0].get_state()
    if what == 'all negative':
      _same(pre, state, 'a fork of no env changed the state')
    for q, c in enumerate(ctxs[1:], 1):
      _same(state, c.get_state(), f'{what}: state of context {q}')
    m = src >= 0
    np.testing.assert_array_equal(state[1][:, R.I_ENV_ID], ENV_ID0 + np.arange(n), err_msg=f'{what}: every env keeps its id')
    np.testing.assert_array_equal(state[0][m], state[0][src[m]], err_msg=f'{what}: a copy equals its source')
    steps(1, 0)
    if not doggo and m.all():   # both copies of the busy bit are set: the first step of a copy runs in the busy kernel
      assert pairs[0][0].busy_count() == n, f'{what}: busy envs of the first step after the fork'
    steps(1 if doggo else 2, None)
  steps(3 if doggo else 8, None)
  # the layout store: sag_reset of forked envs in A against the control given the model's rows with sag_set_layout
  ids = rng.choice(n, size=9, replace=False).astype(np.int32)
  for a, b in pairs:
    b.set_layout(lay[0][ids], lay[1][ids], env_ids=ids)
    a.reset(ids)
    b.reset(ids)
  state = ctxs[0].get_state()
  want_i = lay[1][ids].copy()
  want_i[:, R.I_EPISODE] += 1
  np.testing.assert_array_equal(state[0][ids], lay[0][ids], err_msg='sag_reset of forked envs: floats of the sources\' layouts')
  np.testing.assert_array_equal(state[1][ids], want_i, err_msg='sag_reset of forked envs: ints of the sources\' layouts')
  for q, c in enumerate(ctxs[1:], 1):
    _same(state, c.get_state(), f'sag_reset of forked envs: state of context {q}')
  steps(2, 0)
  for d in devs:
    d.free()
  for c in ctxs:
    c.close()


@pytest.mark.gpu
def test_rejections_are_per_env(nat, monkeypatch):
  """In one context: a chain a <- b <- c (a is rejected: its source b is overwritten), an index == n_envs, INT32_MAX.  Rejected
  and untouched envs keep their state bit for bit, committed ones are as through the host; the following outputs equal the
  control's, the counters are exact, and a rejected env keeps its row of the layout store."""
  n = 203 if HOSTEMU else 1500
  (A, B), descs, doe = _contexts(nat, monkeypatch, [{'SAG_SPLIT': '1'}, {'SAG_SPLIT': '1'}], 'point', list(range(14)), n, None)
  for c in (A, B):
    assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  rng = np.random.RandomState(17)
  state = A.get_state()
  for t in range(5):
    act = _actions('point', *state, rng, t)
    out = A.step(act)[:5]
    _same(out, B.step(act)[:5], f'step {t}')
    state = A.get_state()
  src = np.full(n, -1, np.int32)
  a, b, c_ = 10, 70, 130
  src[a], src[b] = b, c_
  src[3], src[64], src[n - 1] = n, INT32_MAX, n + 1
  src[20:30] = 5          # ordinary copies, and two more chains through them
  src[40] = 21            # (21 is overwritten: rejected)
  src[150:160] = np.arange(150, 160)   # copies onto themselves
  src[161] = 150          # (150 is a copy onto itself: a valid source)
  ok = _rule_ok(src, n, True)
  rejected = (src >= 0) & ~ok
  assert rejected[[a, 3, 64, n - 1, 40]].all() and rejected.sum() == 5 and ok[[b, 161]].all()
  d = _DevSrc(A)
  A.fork_device(d(src))
  assert A.fork_counts() == (int(ok.sum()), 5)
  post = A.get_state()
  np.testing.assert_array_equal(post[0][~ok], state[0][~ok], err_msg='floats of a rejected or untouched env changed')
  np.testing.assert_array_equal(post[1][~ok], state[1][~ok], err_msg='ints of a rejected or untouched env changed')
  _host_fork(B, np.where(ok, src, -1))
  _same(post, B.get_state(), 'state after the fork')
  for t in range(5, 9):
    act = _actions('point', *post, rng, t)
    _same(A.step(act)[:5], B.step(act)[:5], f'step {t}: outputs')
    post = A.get_state()
    _same(post, B.get_state(), f'step {t}: state')
    if t > 5:
      assert A.busy_count() == B.busy_count()
  ids = np.flatnonzero(rejected).astype(np.int32)
  A.reset(ids); B.reset(ids)
  _same(A.get_state(), B.get_state(), 'sag_reset of the rejected envs: their own layouts')
  assert A.fork_counts(clear=True) == (int(ok.sum()), 5) and A.fork_counts() == (0, 0)
  d.free(); A.close(); B.close()


@pytest.mark.gpu
def test_random_streams_of_a_copy(nat, monkeypatch):
  """Without the flag a copy keeps its env id and draws its own action noise.  With SAG_FORK_SAME_STREAM source and copy stay
  bit-identical in the five outputs and the state for 10 steps under equal action rows, through a step that meets and re-draws
  the goal and through a masked sag_reset_device_async of both; W, stepped alike and never forked, holds what the sources
  must hold: the copy differs from W's source row in nothing, and without the flag in SAG_I_ENV_ID alone."""
  n = 203 if HOSTEMU else 1500
  tids = [_tid('go_to_goal'), _tid('catch_goal'), _tid('press_buttons')]
  (A, W), descs, doe = _contexts(nat, monkeypatch, [{'SAG_SPLIT': '1'}, {'SAG_SPLIT': '1'}], 'point', tids, n, None,
                                 config={'action_noise': 0.5})
  for c in (A, W):
    assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  src = (5 * (np.arange(n) // 5)).astype(np.int32)
  lead = src == np.arange(n)
  rng = np.random.RandomState(23)
  dA, dW, d = _DevStep(A), _DevStep(W), _DevSrc(A)

  def step(t, f, i):
    act = _actions('point', f, i, rng, t)[src]
    return dA.step(act), dW.step(act)

  f, i = A.get_state()
  for t in range(3):
    step(t, f, i)
    f, i = A.get_state()
  _same((f, i), W.get_state(), 'two contexts stepped alike')
  A.fork_device(d(src))
  f, i = A.get_state()
  np.testing.assert_array_equal(i[:, R.I_ENV_ID], ENV_ID0 + np.arange(n), err_msg='a copy keeps its own env id')
  wf, wi = W.get_state()
  want_i = wi[src]
  assert (want_i[~lead, R.I_ENV_ID] != i[~lead, R.I_ENV_ID]).all()
  want_i[:, R.I_ENV_ID] = ENV_ID0 + np.arange(n)
  _same((f, i), (wf[src], want_i), 'SAG_I_ENV_ID is the only field a copy does not take')
  step(3, f, i)
  f, i = A.get_state()
  assert (f[~lead] != f[src[~lead]]).any(axis=1).sum() > n // 2, 'copies with their own stream draw their own action noise'
  _same((f[lead], i[lead]), [x[lead] for x in W.get_state()], 'the sources are not touched')
  # the same stream
  f, i = _goals_onto_robots(nat, (A, W), rng)
  A.fork_device(d(src), same_stream=True)
  f, i = A.get_state()
  _same((f, i), [x[src] for x in W.get_state()], 'with the flag a copy takes every field of the record')
  dm, dmw = _DevMask(A), _DevMask(W)
  met = 0
  for t in range(4, 14):
    a, w = step(t, f, i)
    f, i = A.get_state()
    _same(a, [x[src] for x in w], f'step {t}: outputs of source and copy')
    _same((f, i), [x[src] for x in W.get_state()], f'step {t}: state of source and copy')
    met += int(a[4][~lead].sum())
    if t == 8:
      m = ((np.arange(n) // 5) % 3 == 0).astype(np.uint8)   # whole groups
      A.reset_device_async(dm(m), dA.b['obs'])
      W.reset_device_async(dmw(m), dW.b['obs'])
      f, i = A.get_state()
      assert (i[m != 0, R.I_STEP] == 0).all() and A.reset_counts() == (int(m.sum()), 0)
      _same((f, i), [x[src] for x in W.get_state()], 'a masked device reset of sources and copies: the same next layouts')
      _same([dA.get('obs')], [dW.get('obs')[src]], 'first observations of the new episodes')
  assert met > n // 16, 'no copy met its goal: the in-step draws were not exercised'
  for x in (dA, dW, d, dm, dmw):
    x.free()
  A.close(); W.close()


@pytest.mark.gpu
@pytest.mark.parametrize('robot', ['point', 'doggo'])
def test_fork_between_two_contexts(nat, monkeypatch, robot):
  """A source of 3 envs (Doggo: 2), a destination of 130 (70): step_device on the source, the fork and a second step_device
  on the source enqueued without a wait between.  The destination holds the state after the first step (a twin of the source
  stepped synchronously is the reference), the source's second step equals its twin's; then the fork back."""
  ns, nd = (2, 70) if robot == 'doggo' else (3, 130)
  monkeypatch.setenv('SAG_SPLIT', '1')   # (the Doggo has one form)
  tids = CASES['doggo-mixed'][1](nd)[0][:2] if robot == 'doggo' else [_tid('go_to_goal'), _tid('press_buttons'), _tid('push_box')]
  S, descs, _ = _make(nat, robot, tids, ns)
  T, _, _ = _make(nat, robot, tids, ns)
  D, _, _ = _make(nat, robot, tids, nd)
  for c in (S, T, D):
    assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  _same(S.get_state(), T.get_state(), 'source and twin')
  rng = np.random.RandomState(31)
  nu = S.info['nu']
  for t in range(3):
    act = rng.uniform(-1, 1, (ns, nu)).astype(np.float32) * (0 if robot == 'doggo' and t < 2 else 1)
    S.step(act); T.step(act)
  for _ in range(2):   # (the source has taken three steps: the two contexts read different copies of the busy bit)
    D.step(rng.uniform(-1, 1, (nd, nu)).astype(np.float32))
  src = rng.randint(0, ns, nd).astype(np.int32)
  src[7] = -1
  kept = [x[7].copy() for x in D.get_state()]
  a1, a2 = (rng.uniform(-1, 1, (ns, nu)).astype(np.float32) for _ in range(2))
  dS, d = _DevStep(S), _DevSrc(D)
  p = d(src)
  b2 = {k: S.dev_alloc(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (shape, dt) in dS.shapes.items()}
  S.dev_upload(b2['act'], a2)
  dS.enqueue(a1)
  D.fork_device(p, S)
  S.step_device(b2['act'], None, -1, b2['obs'], b2['rew'], b2['cost'], b2['done'], b2['met'])
  D.wait(); S.wait()
  out1 = T.step(a1)[:5]
  tf, ti = T.get_state()
  _same([dS.get(k) for k in ('obs', 'rew', 'cost', 'done', 'met')], out1, 'first step of the source')
  f, i = D.get_state()
  m = src >= 0
  want_i = ti[src[m]].copy()
  want_i[:, R.I_ENV_ID] = ENV_ID0 + np.flatnonzero(m)
  _same((f[m], i[m]), (tf[src[m]], want_i), 'the destination holds the state after the first step')
  _same((f[7], i[7]), kept, 'an env with a negative source')
  assert D.fork_counts() == (nd - 1, 0)
  out2 = T.step(a2)[:5]
  _same([S.dev_download(b2[k], *dS.shapes[k]) for k in ('obs', 'rew', 'cost', 'done', 'met')], out2, 'second step of the source')
  _same(S.get_state(), T.get_state(), 'the source after its second step')
  # the copies step as a context given their records does
  tw = _twin(nat, D)
  act = rng.uniform(-1, 1, (nd, nu)).astype(np.float32)
  _same(D.step(act)[:5], tw.step(act)[:5], 'step of the destination')
  assert robot == 'doggo' or D.busy_count() >= nd - 1, 'the first step of a copy runs in the busy kernel'
  _same(D.get_state(), tw.get_state(), 'state of the destination one step on')
  tw.close()
  # back: destination -> source
  back = np.array([nd - 1, -1] if ns == 2 else [nd - 1, -1, 64], np.int32)
  df, di = D.get_state()
  sf, si = S.get_state()
  d2 = _DevSrc(S)
  S.fork_device(d2(back), D)
  assert S.fork_counts() == (ns - 1, 0)
  f, i = S.get_state()
  mb = back >= 0
  want_i = np.where(mb[:, None], di[back], si)
  want_i[:, R.I_ENV_ID] = ENV_ID0 + np.arange(ns)
  _same((f, i), (np.where(mb[:, None], df[back], sf), want_i), 'fork back into the source')
  tw = _twin(nat, S)
  act = rng.uniform(-1, 1, (ns, nu)).astype(np.float32)
  _same(S.step(act)[:5], tw.step(act)[:5], 'step of the source after the fork back')
  tw.close()
  for x in b2.values():
    S.dev_free(x)
  dS.free(); d.free(); d2.free()
  for c in (S, T, D):
    c.close()


@pytest.mark.gpu
def test_fork_refusals_of_the_c_call(nat):
  """SAG_ERR_ARG (-1) / SAG_ERR_STATE (-4), each with the destination's state and counters untouched."""
  n = 67
  tids = [_tid('go_to_goal'), _tid('press_buttons')]
  D, descs, doe = _make(nat, 'point', tids, n)
  assert D.reset_device(True, episode0=EPISODE0)[0] == 0
  D.step(np.zeros((n, 2), np.float32))
  before = D.get_state()
  d = _DevSrc(D)
  p = d(np.zeros(n, np.int32))

  def refused(code, source, ptr=p, **kw):
    with pytest.raises(nat.SagError, match=rf'\({code}\)'):
      D.fork_device(ptr, source, **kw)
    _same(before, D.get_state(), 'state after a refused fork')
    assert D.fork_counts() == (0, 0)

  car, _, _ = _make(nat, 'car', tids, 5)
  assert car.reset_device(True, episode0=EPISODE0)[0] == 0
  refused(-1, car)                                   # another robot
  rec_f, rec_i = before[0][:5].copy(), before[1][:5].copy()
  rec_i[:, R.I_NV] = np.minimum(rec_i[:, R.I_NV], 4)
  assert (rec_i[:, nat.I_BOX_KIND] == 0).all()
  small = nat.Context('point', 5, seed=KEY, max_vases=4)
  small.set_state(rec_f, rec_i)
  refused(-1, small)                                 # other capacities
  nobox = nat.Context('point', 5, seed=KEY, has_box=False)
  nobox.set_state(rec_f, rec_i)
  refused(-1, nobox)
  empty, _, _ = _make(nat, 'point', tids, 5)
  refused(-4, empty)                                 # no layout in the source
  with pytest.raises(nat.SagError, match=r'\(-4\)'):
    empty.fork_device(d(np.zeros(n, np.int32)), D)   # ... in the destination
  plain = nat.Context('point', 5, seed=KEY)
  plain.set_state(before[0][:5], before[1][:5])
  refused(-4, plain)                                 # tasks on the destination only
  other, _, _ = _make(nat, 'point', tids[::-1], 5)
  assert other.reset_device(True, episode0=EPISODE0)[0] == 0
  refused(-1, other)                                 # differing descriptor tables
  refused(-1, None, flags=2)                         # unknown flag bits
  refused(-1, None, flags=3)
  refused(-1, None, ptr=None)                        # NULL d_src
  # tasks on the source only is served: the state travels, the descriptor index has nowhere to go
  dp = _DevSrc(plain)
  plain.fork_device(dp(np.arange(5, dtype=np.int32)), D)
  assert plain.fork_counts() == (5, 0)
  f, i = plain.get_state()
  _same((f, np.delete(i, R.I_ENV_ID, 1)), (before[0][:5], np.delete(before[1][:5], R.I_ENV_ID, 1)), 'into a context without tasks')
  d.free(); dp.free()
  for c in (D, car, small, nobox, empty, plain, other):
    c.close()


@pytest.mark.gpu
def test_accumulators_and_descriptor_follow_the_fork(nat, monkeypatch):
  """episode_track for a few steps, then a fork: a copy's next finished episode row is what its source's accumulators imply
  (a NumPy tracker permuted alike), rejected envs keep theirs.  Mixed tasks: a forked env then reset by
  sag_reset_device_async carries its source's SAG_I_TASK and the layout the restatement draws for that task."""
  n = 203 if HOSTEMU else 1500
  tids = [_tid('go_to_goal'), _tid('press_buttons'), _tid('push_box'), _tid('collect')]
  (A,), descs, doe = _contexts(nat, monkeypatch, [{'SAG_SPLIT': '1'}], 'point', tids, n, None)
  assert A.reset_device(True, episode0=EPISODE0)[0] == 0
  dv, d, dm = _DevStep(A), _DevSrc(A), _DevMask(A)
  ended_p, episode_p = A.dev_alloc(n), A.dev_alloc(16 * n)
  A.dev_upload(episode_p, np.zeros((n, 4), np.float32))
  acc, episode = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
  rng = np.random.RandomState(41)
  limit = 9

  def step(t):
    f, i = A.get_state()
    out = dv.step(_actions('point', f, i, rng, t))
    A.episode_track(dv.b['rew'], dv.b['cost'], dv.b['done'], dv.b['met'], limit, ended_p, episode_p)
    A.wait()
    ended = _track_ref(acc, out[1], out[2], out[3], out[4], limit, episode)
    np.testing.assert_array_equal(A.dev_download(ended_p, (n,), np.uint8), ended, err_msg=f'step {t}: ended')
    np.testing.assert_array_equal(A.dev_download(episode_p, (n, 4), np.float32), episode, err_msg=f'step {t}: episode rows')
    return ended

  for t in range(4):
    step(t)
  src = np.where(np.arange(n) % 7 == 0, -1, 7 * (np.arange(n) // 7)).astype(np.int32)   # env 7k+1 .. 7k+6 from env 7k, of another task
  src[5] = n   # rejected
  ok = _rule_ok(src, n, True)
  assert (acc[:, 2] == 4).all() and (acc[:, 0] != 0).sum() > n // 2 and (doe[src[ok]] != doe[ok]).any()
  A.fork_device(d(src))
  assert A.fork_counts() == (int(ok.sum()), 1)
  acc[ok] = acc[src[ok]]
  doe = doe.copy()
  doe[ok] = doe[src[ok]]
  seen = set()
  for t in range(4, 4 + limit):
    seen |= set(step(t).tolist())
  assert 2 in seen, 'no episode reached the limit: the copied lengths were not exercised'
  # a masked device reset of forked envs: the source's descriptor
  m = (np.arange(n) % 3 == 1)
  pre = A.get_state()
  np.testing.assert_array_equal(pre[1][:, R.I_TASK], np.asarray(tids)[doe], err_msg='SAG_I_TASK of the copies')
  A.reset_device_async(dm(m.astype(np.uint8)), None)
  post = A.get_state()
  assert A.reset_counts() == (int(m.sum()), 0)
  _expect_reset('point', descs, doe, _cfg(), ENV_ID0 + np.arange(n), KEY, pre, post, m)
  A.dev_free(ended_p); A.dev_free(episode_p)
  dv.free(); d.free(); dm.free(); A.close()


def _env_outputs(out):
  return [_np(out[0]), _np(out[1]), _np(out[2]) != 0, _np(out[3]['cost']) != 0, _np(out[3]['goal_met']) != 0, out[3]['bound']]


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [{}, {'device_buffers': True}, {'devices': [0, 0]}, {'device_buffers': True, 'devices': [0, 0]}],
                         ids=['host buffers', 'device buffers', 'devices=[0, 0]', 'device buffers, devices=[0, 0]'])
def test_env_fork(nat, kw):
  """env.fork(src) with a host src, a device src and source=other beside an env moved by hand with get_state / set_state:
  info['bound'] (random_bound), the last observation rows of host-buffer mode and the next steps."""
  n = 130 if HOSTEMU else 1000
  config = {'random_bound': 1}
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=37, config=config, **kw)
  ref = _make_env('point', 'go_to_goal', n_envs=n, seed=37, config=config)
  np.testing.assert_array_equal(_np(env.reset()), ref.reset())
  rng = np.random.RandomState(3)
  ranges = env._ranges
  bound0 = ref._bounds.copy()
  assert len(np.unique(bound0)) > n // 2

  def step(what):
    act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    a, b = env.step(act), ref.step(act)
    _same(_env_outputs(a), _env_outputs(b), what)
    _same(env.get_state(), ref.get_state(), f'{what}: state')
    return b

  def by_hand(src, source=None):
    sf, si = (source or ref).get_state()
    f, i = ref.get_state()
    m = src >= 0
    own = i[:, R.I_ENV_ID].copy()
    f[m], i[m] = sf[src[m]], si[src[m]]
    i[:, R.I_ENV_ID] = own
    ref.set_state(f, i)
    ref._bounds = f[:, R.F_BOUND].copy()

  def shard_src():
    """groups of 5 inside every shard, some envs kept"""
    src = np.full(n, -1, np.int64)
    for s, e in ranges:
      src[s:e] = s + 5 * ((np.arange(s, e) - s) // 5)
    src[rng.rand(n) < 0.2] = -1
    return src   # (a leader that is kept is a valid source)

  for _ in range(2):
    last = step('before the fork')
  src = shard_src()
  env.fork(src)
  by_hand(src)
  m = src >= 0
  assert env.fork_counts(clear=True) == (int(m.sum()), 0)
  _same(env.get_state(), ref.get_state(), 'state after fork(host src)')
  np.testing.assert_array_equal(env._bounds, ref._bounds)
  assert (env._bounds[m] == bound0[src[m]]).all() and (env._bounds != bound0).any()
  if not kw.get('device_buffers'):
    want = last[0].copy()
    want[m] = last[0][src[m]]
    np.testing.assert_array_equal(env._last_obs, want, err_msg='the last observation rows follow the fork')
  for k in range(2):
    step(f'step {k} after fork(host src)')
  # a device src: shard-local indices, one array per shard
  src = shard_src()
  bufs = []
  for c, (s, e) in zip(env._ctx, ranges):
    p = c.dev_alloc(4 * (e - s))
    c.dev_upload(p, np.where(src[s:e] < 0, -1, src[s:e] - s).astype(np.int32))
    bufs.append((c, p, nat.DeviceArray(c, p.value, (e - s,), np.int32)))
  env.fork([b[2] for b in bufs] if len(bufs) > 1 else bufs[0][2])
  by_hand(src)
  assert env.fork_counts(clear=True) == (int((src >= 0).sum()), 0)
  _same(env.get_state(), ref.get_state(), 'state after fork(device src)')
  np.testing.assert_array_equal(env._bounds, ref._bounds)
  step('step after fork(device src)')
  for c, p, _ in bufs:
    c.dev_free(p)
  # source=other: a snapshot env of the same shape, saved into and restored from
  snap = _make_env('point', 'go_to_goal', n_envs=n, seed=99, config=config, **kw)
  snap.reset()
  snap.fork(np.arange(n), source=env)
  saved = ref.get_state()
  saved_bounds = ref._bounds.copy()
  for k in range(2):
    step(f'step {k} after the snapshot')
  sf, si = snap.get_state()
  own = si[:, R.I_ENV_ID].copy()
  np.testing.assert_array_equal(own, np.arange(n))
  _same((sf, si), saved, 'the snapshot holds the state at the fork')
  np.testing.assert_array_equal(snap._bounds, saved_bounds)
  back = np.where(rng.rand(n) < 0.5, np.arange(n), -1)
  env.fork(back, source=snap)
  by_hand(back, source=snap)
  _same(env.get_state(), ref.get_state(), 'state after the restore')
  step('step after the restore')
  env.close(); ref.close(); snap.close()


@pytest.mark.gpu
def test_env_fork_refusals_and_time_limit(nat):
  """Every ValueError of fork(), with nothing changed; and with time_limit the accumulators follow the fork: a copy is
  truncated when its source is."""
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import benchmark
  n = 40
  for kw in ({}, {'device_buffers': True}, {'parity_rng': True}):
    plain = sag.make('point', 'go_to_goal', n_envs=n, seed=5, **kw)
    plain.reset()
    with pytest.raises(ValueError):
      plain.fork(np.zeros(n, int))
    plain.close()
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=5, devices=[0, 0])
  env.reset()
  env.step(np.zeros((n, 2), np.float32))
  before = env.get_state()
  chain = np.full(n, -1); chain[1], chain[2] = 2, 3
  cross = np.full(n, -1); cross[0] = n - 1
  car = _make_env('car', 'go_to_goal', n_envs=n, seed=5, devices=[0, 0])
  other_task = _make_env('point', 'press_buttons', n_envs=n, seed=5, devices=[0, 0])
  other_cfg = _make_env('point', 'go_to_goal', n_envs=n, seed=5, devices=[0, 0], config={'hazards_size': 0.3})
  one = _make_env('point', 'go_to_goal', n_envs=n, seed=5)
  unset = sag.make('point', None, n_envs=n, seed=5, device_reset=True, devices=[0, 0])
  for e in (car, other_task, other_cfg, one):
    e.reset()
  c0 = env._ctx[0]
  p = c0.dev_alloc(4 * n)
  bad = [(np.zeros(n - 1, int), {}), (np.zeros((n, 1), int), {}), (np.zeros(n, np.float32), {}), (np.zeros(n, bool), {}),
         (np.full(n, n), {}), (chain, {}), (cross, {}), (np.zeros(n, int), {'source': car}), (np.zeros(n, int), {'source': other_task}),
         (np.zeros(n, int), {'source': other_cfg}), (np.zeros(n, int), {'source': one}), (np.zeros(n, int), {'source': unset}),
         (nat.DeviceArray(c0, p.value, (n // 2,), np.int32), {}),                                # one device src for two shards
         ([nat.DeviceArray(c0, p.value, (n // 2,), np.float32)] * 2, {}), ([nat.DeviceArray(c0, p.value, (n // 2 - 1,), np.int32)] * 2, {})]
  for src, kw in bad:
    with pytest.raises(ValueError):
      env.fork(src, **kw)
  _same(before, env.get_state(), 'state after refused forks')
  assert env.fork_counts() == (0, 0)
  c0.dev_free(p)
  for e in (env, car, other_task, other_cfg, one, unset):
    e.close()
  # time_limit: env 1 .. 4 take env 0's accumulators after 3 of 5 steps, then an older env's after a reset
  limit = 5
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True, time_limit=limit)
  env.reset()
  zero = np.zeros((n, 2), np.float32)
  for _ in range(3):
    env.step(zero)
  young = np.arange(n) >= n // 2
  env.reset(mask=young)   # their episodes start over
  src = np.full(n, -1); src[n // 2:n // 2 + 5] = 0; src[1] = n - 1
  env.fork(src)
  length = np.where(young, 0, 3)
  length[src >= 0] = length[src[src >= 0]]
  for k in range(1, 6):
    obs, rew, ended, info = env.step(zero)
    length += 1
    e, term = _np(ended), _np(info['terminated']) != 0
    np.testing.assert_array_equal(e == 2, (length == limit) & ~term, err_msg=f'step {k}: truncated envs')
    np.testing.assert_array_equal(_np(info['episode'])[e != 0, 2], length[e != 0])
    length[e != 0] = 0
  env.close()

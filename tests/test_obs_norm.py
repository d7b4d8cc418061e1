"""Observation normalisation on the device (csrc/sag_obs_norm.hpp and the NORM instances of csrc/sag_policy.hpp and
csrc/sag_policy_grad.hpp: sag_obs_stats_device, sag_policy_forward_norm_device, sag_policy_backward_norm_device, and
sag.MLPPolicy(normalize_observations=True) with sag.PPOLearner) against the NumPy restatement of tests/obs_norm_ref.py, which
test_obs_norm_ref.py pins - never against the kernels' own arithmetic.

The moments are defined to a tolerance.  Per case the error of the float32 restatement (column sums one row after the other,
against the float64 one) is computed per column - the mean's on the scale of the column's deviation, M2's relatively - and the
device is granted 8 times the largest over the columns: it adds the same fp32 terms in another order.  Columns have scales
from 1e-3 to 1e3 and means of their own, so a wrong column mapping misses by orders of magnitude.  Where a tolerance could hide a
dropped row the exact cases take over: integers in -2 ... 2 make every fp32 partial exact, so count and mean must be the
integers' own; a constant column must give M2 == 0.  Given its state the table is defined bit for bit, and every case checks
it against table32 of the device's own state.  The normalised forward and backward are compared bit for bit with the PLAIN
entry points run on normalize32(obs) uploaded from the host.  Shapes: a block's unit is 1024 rows, so one row, 33 x 3 pitched,
2049 rows on two blocks (three chunks) and 1025 x 3 (planes end inside a chunk).  The kernel cases also run on the host build
of the device sources (test_obs_norm_hostemu.py).

A rollout's rows have columns that are constant in every batch; after a merge their M2 is rounding noise of the means, which
obs_norm_ref.resolved() keeps out of the relative measure and near_constant_ok() bounds by n 2^-24 |mean|.  The measured errors
are in the docstring of test_stats_against_the_reference and in DESIGN 3.11."""
import ctypes as C
import os

import numpy as np
import pytest

import obs_norm_ref as O
import policy_grad_ref as G
import policy_ref as P
from test_device_reset import KEY

F32, F64 = np.float32, np.float64
HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
ERR_ARG, ERR_UNSUPPORTED = -1, -5
TABLE_ONLY = 1
GUARD = 8
SENTINEL = 7.0
FACTOR = 8.0
EPS = 1e-8
ROBOTS = {'point': (60, 2), 'car': (72, 2), 'doggo': (104, 12)}


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


class _Buf:
  """A device buffer that holds exactly `host` (any dtype), freed by free()."""

  def __init__(self, c, host):
    self.c, self.host = c, np.ascontiguousarray(host)
    self.p = c.dev_alloc(max(self.host.nbytes, 16))
    c.dev_upload(self.p, self.host)

  def get(self):
    return self.c.dev_download(self.p, self.host.shape, self.host.dtype)

  def free(self):
    self.c.dev_free(self.p)


# ----------------------------------------------------------------------------------------------------------------------
# sag_obs_stats_device
# ----------------------------------------------------------------------------------------------------------------------
def _values(rng, rows, od):
  """[rows, od] float32: column k has deviation 10^(-3 ... 3) and a mean of 0.5 ... 2 deviations of either sign."""
  r = np.random.RandomState(od)   # the columns' scales belong to the robot, not to the batch
  scale = 10.0**r.permutation(np.linspace(-3, 3, od))
  mean = scale * r.uniform(0.5, 2.0, od) * r.choice([-1.0, 1.0], od)
  return (mean + scale * rng.normal(size=(rows, od))).astype(F32)


def _layout(values, n_rows, n_planes, pitch, obs_pitch):
  """The logical rows [n_planes * n_rows, od] at (p * pitch + r) * obs_pitch, NaN in every pad row and pad column; the array
  ends with the last counted row's last column."""
  od = values.shape[1]
  x = np.full(((n_planes - 1) * pitch + n_rows - 1) * obs_pitch + od, np.nan, F32)
  idx = (np.arange(n_planes)[:, None] * pitch + np.arange(n_rows)[None, :]).reshape(-1)
  x[(idx[:, None] * obs_pitch + np.arange(od)[None, :])] = values
  return x


class _Stats:
  """A state and a table on the device with guard words behind both; call() is one sag_obs_stats_device and returns the
  downloaded (state, table) after checking the guards and that the table is table32 of the device's own state, bit for bit."""

  def __init__(self, c, od, state=None, eps=EPS):
    self.c, self.od, self.eps = c, od, eps
    s = np.full(1 + 2 * od + GUARD, SENTINEL, F64)
    s[:1 + 2 * od] = O.empty_state(od) if state is None else state
    self.state, self.table = _Buf(c, s), _Buf(c, np.full(2 * od + GUARD, SENTINEL, F32))

  def raw(self, desc):
    rc = self.c.lib.sag_obs_stats_device(self.c.h, C.byref(desc) if desc is not None else None)
    self.c.wait()
    return rc

  def desc(self, nat, d_obs, n_rows, n_planes, pitch, obs_pitch, max_blocks=0, flags=0):
    return nat.ObsStatsDesc(n_rows, n_planes, pitch, obs_pitch, max_blocks, flags, self.eps, 0.0, d_obs, self.state.p.value, self.table.p.value)

  def get(self, check_table=True):
    od = self.od
    s, t = self.state.get(), self.table.get()
    assert (s[1 + 2 * od:] == SENTINEL).all() and (t[2 * od:] == F32(SENTINEL)).all(), 'a write behind the state or the table'
    state, table = s[:1 + 2 * od], t[:2 * od].reshape(2, od)
    if check_table:
      assert table.tobytes() == O.table32(state, self.eps).tobytes(), 'the table is not table32 of the device\'s own state'
    return state, table

  def call(self, nat, values, n_rows, n_planes, pitch, obs_pitch, max_blocks=0):
    x = _Buf(self.c, _layout(values, n_rows, n_planes, pitch, obs_pitch))
    rc = self.raw(self.desc(nat, x.p.value, n_rows, n_planes, pitch, obs_pitch, max_blocks))
    assert rc == 0, self.c.lib.sag_last_error(self.c.h)
    x.free()
    return self.get()

  def free(self):
    self.state.free(); self.table.free()


def _within(state, batches, what, start=None):
  """The device's state after `batches` (in that order, from the empty state or from `start`) against the float64 restatement,
  under FACTOR times the float32 restatement's own error."""
  od = batches[0].shape[1]
  ref = own = O.empty_state(od) if start is None else np.asarray(start, F64)
  for b in batches:
    ref, own = O.merge(ref, O.batch_moments(b)), O.merge(own, O.batch_moments(b, F32))
  cols = O.resolved(ref)   # every column of the synthetic cases; a rollout's rows have constant columns (near_constant_ok)
  e_own, e = O.measure(own, ref, cols), O.measure(state, ref, cols)
  tol = FACTOR * max(e_own.values())
  print(f'{what}: tolerance {tol:.3e}, restatement mean {e_own["mean"]:.2e} M2 {e_own["M2"]:.2e}, device mean {e["mean"]:.2e} M2 {e["M2"]:.2e}'
        f' over {int(cols.sum())} of {od} columns')
  assert cols.sum() >= od // 2 and O.near_constant_ok(state, ref), f'{what}: a near-constant column is off'
  assert state[0] == ref[0], f'{what}: count {state[0]} for {ref[0]}'
  bad = {k: v for k, v in e.items() if not v <= tol}
  assert not bad, f'{what}: {bad} beyond {tol:.3e}'


# (name, n_rows, n_planes, pitch, max_blocks)
STAT_SHAPES = [('33 x 3 pitched', 33, 3, 38, 0), ('one row', 1, 1, 1, 0), ('2049 rows, three chunks on two blocks', 2049, 1, 2049, 2),
               ('1025 x 3, planes end inside a chunk', 1025, 3, 1025, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
@pytest.mark.parametrize('case', range(len(STAT_SHAPES)), ids=[s[0] for s in STAT_SHAPES])
def test_stats_against_the_reference(nat, ctxs, robot, case):
  """mean and M2 of every column within 8 x the float32 restatement's own error, the count exact, obs_pitch = obs_dim + 4 with
  NaN in every pad row and pad column, nothing written behind the state or the table, the table bit for bit.
  Measured on the MI355X, largest over the robots, device / float32 restatement (mean, M2): 33 x 3 2.5e-7, 1.6e-7 / 8.6e-7,
  4.2e-7; one row exact; 2049 rows on two blocks 3.7e-7, 1.3e-7 / 3.2e-6, 2.0e-6; 1025 x 3 2.0e-7, 1.2e-7 / 4.1e-6, 2.1e-6 - the
  device is below the restatement's own error in every case."""
  name, n_rows, n_planes, pitch, mb = STAT_SHAPES[case]
  c = ctxs(robot)
  od = ROBOTS[robot][0]
  values = _values(np.random.RandomState(100 + case), n_rows * n_planes, od)
  st = _Stats(c, od)
  state, table = st.call(nat, values, n_rows, n_planes, pitch, od + 4, mb)
  _within(state, [values], f'{robot}, {name}')
  assert np.isfinite(table).all()
  st.free()


@pytest.mark.gpu
@pytest.mark.parametrize('robot,n_rows,n_planes,pitch,mb', [('point', 33, 3, 38, 0), ('car', 2049, 1, 2049, 2), ('doggo', 1025, 3, 1030, 0)])
def test_stats_exact_on_small_integers_and_constants(nat, ctxs, robot, n_rows, n_planes, pitch, mb):
  """Integers in -2 ... 2: every fp32 partial sum is an integer below 2^24 and exact whatever the order, so count == n and
  mean == sum / n in float64 exactly, per column (a row dropped or taken twice moves a column's sum).  Column 0 is the
  constant 1.5: mean 1.5, M2 0 and rstd = float32(1 / sqrt(eps)) exactly."""
  c = ctxs(robot)
  od = ROBOTS[robot][0]
  n = n_rows * n_planes
  k = np.random.RandomState(n_rows).randint(-2, 3, (n, od)).astype(F64)
  k[:, 0] = 1.5
  st = _Stats(c, od)
  state, table = st.call(nat, k.astype(F32), n_rows, n_planes, pitch, od + 4, mb)
  assert state[0] == n
  np.testing.assert_array_equal(state[1:1 + od], k.sum(axis=0) / F64(n))
  assert state[1] == 1.5 and state[1 + od] == 0.0
  assert table[0][0] == F32(1.5) and table[1][0] == F32(1.0 / np.sqrt(F64(F32(EPS))))
  _within(state, [k.astype(F32)], f'{robot} integers')
  st.free()


@pytest.mark.gpu
def test_stats_state_handling(nat, ctxs):
  """Three successive calls on 7, 33 and 130 rows agree with the moments of the concatenation; the empty state gives the
  identity table; TABLE_ONLY leaves every state byte and reproduces the table's bits; the same call from the same state gives
  the same bits."""
  c = ctxs('car')
  od = ROBOTS['car'][0]
  rng = np.random.RandomState(5)
  batches = [_values(rng, n, od) for n in (7, 33, 130)]
  st = _Stats(c, od)
  assert st.raw(st.desc(nat, None, 0, 0, 0, 0, flags=TABLE_ONLY)) == 0
  state, table = st.get()
  assert not state.any()
  np.testing.assert_array_equal(table, np.stack([np.zeros(od, F32), np.ones(od, F32)]))
  states = []
  for b in batches:
    state, table = st.call(nat, b, len(b), 1, len(b), od + 4)
    states.append(state.copy())
  _within(state, batches, '7 + 33 + 130 rows')
  x = np.concatenate(batches).astype(F64)
  assert state[0] == 170
  std = x.std(axis=0)
  assert (np.abs(state[1:1 + od] - x.mean(axis=0)) <= 1e-5 * std).all() and (np.abs(state[1 + od:] / 170 - x.var(axis=0)) <= 1e-5 * x.var(axis=0)).all()
  # TABLE_ONLY from that state: the table cleared first, then rewritten with the same bits; the state's bytes stay
  st.table.c.dev_upload(st.table.p, np.full(2 * od + GUARD, SENTINEL, F32))
  assert st.raw(st.desc(nat, None, 0, 0, 0, 0, flags=TABLE_ONLY)) == 0
  state2, table2 = st.get()
  assert state2.tobytes() == state.tobytes() and table2.tobytes() == table.tobytes()
  # the last call again from the state before it: the same bits
  again = _Stats(c, od, state=states[1])
  s3, t3 = again.call(nat, batches[2], 130, 1, 130, od + 4)
  assert s3.tobytes() == state.tobytes() and t3.tobytes() == table.tobytes()
  st.free(); again.free()


@pytest.mark.gpu
def test_stats_refusals_enqueue_nothing(nat, ctxs):
  c = ctxs('point')
  od = ROBOTS['point'][0]
  values = _values(np.random.RandomState(1), 33 * 3, od)
  x = _Buf(c, _layout(values, 33, 3, 38, od + 4))
  st = _Stats(c, od, state=np.arange(1 + 2 * od, dtype=F64) + 1)
  good = dict(n_rows=33, n_planes=3, pitch=38, obs_pitch=od + 4, max_blocks=0, flags=0)
  bad = [dict(n_rows=0), dict(n_rows=-1), dict(n_planes=0), dict(pitch=32), dict(n_rows=1 << 16, n_planes=1 << 15, pitch=1 << 16),
         dict(obs_pitch=od - 4), dict(obs_pitch=od + 2), dict(max_blocks=-1), dict(flags=2), dict(flags=-1), dict(eps=0.0), dict(eps=-1e-8),
         dict(eps=float('nan')), dict(eps=float('inf')), dict(d_obs=None), dict(d_state=None), dict(d_table=None),
         dict(d_obs=x.p.value + 8), dict(d_state=st.state.p.value + 4), dict(d_table=st.table.p.value + 8),
         dict(flags=TABLE_ONLY, d_state=None), dict(flags=TABLE_ONLY, eps=0.0), dict(flags=TABLE_ONLY | 4)]
  before = st.state.get().tobytes(), st.table.get().tobytes()
  for change in bad:
    d = st.desc(nat, x.p.value, **good)
    for k, v in change.items():
      setattr(d, k, v)
    assert st.raw(d) == ERR_ARG, change
    assert c.lib.sag_last_error(c.h).decode().startswith('sag_obs_stats_device:'), change
    assert (st.state.get().tobytes(), st.table.get().tobytes()) == before, f'{change}: refused, but the state or the table was written'
  assert st.raw(None) == ERR_ARG
  assert c.lib.sag_obs_stats_device(None, None) == ERR_ARG
  fresh = _Stats(c, od)   # the context is usable afterwards
  state, _ = fresh.call(nat, values, 33, 3, 38, od + 4)
  _within(state, [values], 'after the refusals')
  x.free(); st.free(); fresh.free()


# ----------------------------------------------------------------------------------------------------------------------
# sag_policy_forward_norm_device / sag_policy_backward_norm_device
# ----------------------------------------------------------------------------------------------------------------------
CLIP = 5.0


def _table(rng, od):
  """mean of either sign, rstd from 1e-2 to 1e2 over the columns."""
  rstd = 10.0**rng.permutation(np.linspace(-2, 2, od))
  mean = rng.uniform(0.5, 2.0, od) * rng.choice([-1.0, 1.0], od) / rstd
  return np.stack([mean, rstd]).astype(F32)


def _raw_obs(rng, rows, table, pad=0):
  """Rows whose normalised values are about N(0, 2^2) - most inside +-CLIP - with one element far beyond either clamp in
  every row; NaN in the pad columns."""
  od = table.shape[1]
  obs = np.full((rows, od + pad), np.nan, F32)
  z = rng.normal(0, 2.0, (rows, od))
  z[:, 3], z[:, od - 2] = 100.0, -100.0
  obs[:, :od] = table[0].astype(F64) + z / table[1].astype(F64)
  ref = O.normalize32(obs[:, :od], table, CLIP)
  assert (ref == F32(CLIP)).any() and (ref == F32(-CLIP)).any() and (np.abs(ref) < CLIP).mean() > 0.9 and np.isfinite(ref).all()
  return obs, ref


def _forward(nat, c, prm, obs, hidden, table=None, clip=CLIP, **kw):
  """One forward on fresh buffers (test_policy._Call) through the plain entry point, or with `table` the _norm one ->
  {output: rows + guard rows}; asserts that rows at and beyond n_rows keep their sentinel."""
  from test_policy import _Call
  k = _Call(nat, c, P.pack(prm), obs, hidden, **kw)
  if table is None:
    rc = k.run()
  else:
    t = _Buf(c, table)
    rc = c.lib.sag_policy_forward_norm_device(c.h, C.byref(k.desc), t.p.value, clip)
    c.wait()
    t.free()
  assert rc == 0, c.lib.sag_last_error(c.h)
  assert k.untouched(), 'a write at or beyond n_rows'
  out = {n: k.get(n) for n in ('actions', 'logp', 'value', 'cvalue')}
  k.free()
  return out


def _same_bits(a, b, what):
  for n in a:
    assert np.isfinite(a[n][:1]).all()
    np.testing.assert_array_equal(a[n].view(np.uint32), b[n].view(np.uint32), err_msg=f'{what}: {n}')


@pytest.mark.gpu
@pytest.mark.parametrize('activation', [0, 1], ids=['relu', 'tanh'])
@pytest.mark.parametrize('hidden', [32, 64] + ([] if HOSTEMU else [256]))
@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
def test_forward_norm_equals_the_plain_forward_on_normalize32(nat, ctxs, robot, hidden, activation):
  """Rows 1, 31, 33 and 65: sampled actions (the same draw), logp, value and cost value of forward_norm(obs) equal the plain
  sag_policy_forward_device on normalize32(obs) uploaded from the host, bit for bit."""
  c = ctxs(robot)
  od, nu = ROBOTS[robot]
  rng = np.random.RandomState(1000 * hidden + od + activation)
  prm = P.random_params(rng, od, nu, hidden, scale=1.5)
  table = _table(rng, od)
  for rows in (1, 31, 33, 65):
    obs, ref = _raw_obs(rng, rows, table)
    kw = dict(activation=activation, draw=11, row0=5, logp_const=P.logp_const(prm['std']))
    got = _forward(nat, c, prm, obs, hidden, table=table, **kw)
    want = _forward(nat, c, prm, ref, hidden, **kw)
    _same_bits(got, want, f'{robot} {hidden} {rows}')
    plain = _forward(nat, c, prm, obs, hidden, **kw)
    assert (plain['value'][:rows] != got['value'][:rows]).any(), 'the normalisation changed nothing'


@pytest.mark.gpu
def test_forward_norm_pitched_nan_pads_and_the_identity(nat, ctxs):
  """obs_pitch = obs_dim + 4 with NaN pad columns, 33 of 40 uploaded rows asked for (the rest NaN throughout); clip = +inf
  under the identity table equals the plain call on obs itself; a NaN observation element passes through to its row's outputs
  (tanh: a ReLU turns a NaN into 0) and to no other row's."""
  c = ctxs('doggo')
  od, nu = ROBOTS['doggo']
  rng = np.random.RandomState(8)
  prm = P.random_params(rng, od, nu, 64)
  table = _table(rng, od)
  obs, ref = _raw_obs(rng, 40, table, pad=4)
  obs[33:] = np.nan
  kw = dict(flags=1, n_rows=33)
  _same_bits(_forward(nat, c, prm, obs, 64, table=table, pitch=od + 4, **kw), _forward(nat, c, prm, ref, 64, **kw), 'pitched')
  ident = np.stack([np.zeros(od, F32), np.ones(od, F32)])
  big = obs[:33, :od] * F32(1e3)
  _same_bits(_forward(nat, c, prm, big, 64, table=ident, clip=float('inf'), draw=2), _forward(nat, c, prm, big, 64, draw=2), 'identity')
  poisoned = obs[:33, :od].copy()
  poisoned[7, 50] = np.nan
  got = _forward(nat, c, prm, poisoned, 64, table=table, flags=1, activation=1)
  assert np.isnan(got['value'][7]) and np.isfinite(np.delete(got['value'][:33], 7)).all()


def _grad_batch(rng, prm, rows, table, activation):
  """policy_grad_ref.make_batch's recipe on given raw observations: actions, old log-probabilities (ratios away from the clip
  edges), advantages and returns that belong to the network's outputs on the NORMALISED rows."""
  obs, ref = _raw_obs(rng, rows, table)
  mean, v, cv = P.forward_ref64(prm, ref, activation)
  actions = (mean + np.asarray(prm['std'], F64) * rng.standard_normal(mean.shape)).astype(F32)
  logp = G.logp64(prm, ref, actions, activation)
  r = np.asarray(G.RATIOS)[rng.randint(0, len(G.RATIOS), rows)]
  batch = dict(obs=obs, actions=actions, logp_old=(logp - np.log(r)).astype(F32), adv=rng.standard_normal(rows).astype(F32),
               ret=(v + rng.standard_normal(rows)).astype(F32), cadv=rng.standard_normal(rows).astype(F32),
               cret=(cv + rng.standard_normal(rows)).astype(F32))
  return batch, ref


def _backward(nat, c, prm, batch, hidden, n_rows, n_planes, pitch, activation, flags, table=None, fill=SENTINEL, max_blocks=0):
  """One backward over the batch laid out as n_planes planes of `pitch` rows with NaN pad rows -> the n_params + 8 words
  (guards checked), through the plain entry point or with `table` the _norm one."""
  from test_policy_grad import _planes
  flat = P.pack(prm)
  n_words = len(flat) + 8
  bufs = {k: _Buf(c, _planes(batch[k], n_rows, n_planes, pitch)) for k in ('obs', 'actions', 'logp_old', 'adv', 'ret', 'cadv', 'cret')}
  bufs['params'] = _Buf(c, flat)
  bufs['grad'] = _Buf(c, np.full(n_words + GUARD, fill, F32))
  co = G.COEF
  p = lambda k: bufs[k].p.value   # noqa: E731
  d = nat.PolicyGradDesc(n_rows, n_planes, pitch, c.info['obs_dim'], hidden, activation, flags, max_blocks, co['clip'], co['vf_coef'], co['cvf_coef'],
                         co['ent_coef'], co['adv_mul'], co['adv_sub'], co['cadv_mul'], co['cadv_sub'], 1.0 / (n_rows * n_planes), 0.0,
                         p('params'), p('obs'), p('actions'), p('logp_old'), p('adv'), p('ret'), p('cadv'), p('cret'), p('grad'))
  if table is None:
    rc = c.lib.sag_policy_backward_device(c.h, C.byref(d))
  else:
    bufs['table'] = _Buf(c, table)
    rc = c.lib.sag_policy_backward_norm_device(c.h, C.byref(d), p('table'), CLIP)
  c.wait()
  assert rc == 0, c.lib.sag_last_error(c.h)
  w = bufs['grad'].get()
  assert (w[n_words:] == F32(fill)).all(), 'a write behind d_grad'
  for b in bufs.values():
    b.free()
  return w[:n_words]


@pytest.mark.gpu
@pytest.mark.parametrize('activation', [0, 1], ids=['relu', 'tanh'])
@pytest.mark.parametrize('hidden', [32] + ([] if HOSTEMU else [128]))
@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
def test_backward_norm_equals_the_plain_backward_on_normalize32(nat, ctxs, robot, hidden, activation):
  """3 planes x 33 rows at pitch 38: all n_params + 8 words of backward_norm(obs) equal the plain sag_policy_backward_device
  on normalize32(obs) bit for bit (the same grid: the same partials in the same order), with and without ACCUMULATE."""
  c = ctxs(robot)
  od, nu = ROBOTS[robot]
  rng = np.random.RandomState(77 * hidden + od + activation)
  prm = P.random_params(rng, od, nu, hidden)
  table = _table(rng, od)
  batch, ref = _grad_batch(rng, prm, 99, table, ('relu', 'tanh')[activation])
  plain_batch = dict(batch, obs=ref)
  for flags, fill in ((0, SENTINEL), (1, 0.25)):   # ACCUMULATE adds to the 0.25 that d_grad holds
    got = _backward(nat, c, prm, batch, hidden, 33, 3, 38, activation, flags, table=table, fill=fill)
    want = _backward(nat, c, prm, plain_batch, hidden, 33, 3, 38, activation, flags, fill=fill)
    assert np.isfinite(got).all() and abs(got[-3] - fill * flags - 1.0) < 1e-5   # statistic 5: every row counted, times scale
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f'{robot} {hidden} flags {flags}')
  raw = _backward(nat, c, prm, batch, hidden, 33, 3, 38, activation, 0)
  assert (raw != got).mean() > 0.5, 'the normalisation changed nothing'


@pytest.mark.gpu
def test_norm_refusals_enqueue_nothing(nat, ctxs):
  """What the plain entry points refuse the _norm ones refuse too (flags = 2 among them), and in addition a NULL or misaligned
  table and a clip that is not above 0; hidden 160 stays SAG_ERR_UNSUPPORTED for the backward.  Outputs keep their fill."""
  from test_policy import _Call
  c = ctxs('point')
  od, nu = ROBOTS['point']
  rng = np.random.RandomState(4)
  prm = P.random_params(rng, od, nu, 32)
  table = _table(rng, od)
  obs, _ = _raw_obs(rng, 33, table)
  t = _Buf(c, np.concatenate([table.reshape(-1), np.zeros(4, F32)]))
  tp = t.p.value
  fwd = c.lib.sag_policy_forward_norm_device
  cases = [({}, None, CLIP), ({}, tp + 8, CLIP), ({}, tp, 0.0), ({}, tp, -1.0), ({}, tp, float('nan')), (dict(flags=2), tp, CLIP),
           (dict(hidden=48), tp, CLIP), (dict(n_rows=0), tp, CLIP), (dict(obs_pitch=od + 2), tp, CLIP), (dict(d_obs=None), tp, CLIP)]
  for change, table_ptr, clip in cases:
    k = _Call(nat, c, P.pack(prm), obs, 32)
    for f, v in change.items():
      setattr(k.desc, f, v)
    assert fwd(c.h, C.byref(k.desc), table_ptr, clip) == ERR_ARG, (change, table_ptr, clip)
    c.wait()
    assert c.lib.sag_last_error(c.h).decode().startswith('sag_policy_forward_norm_device:')
    assert k.untouched(0), f'{change}: refused, but an output was written'
    k.free()
  assert fwd(c.h, None, tp, CLIP) == ERR_ARG and fwd(None, None, tp, CLIP) == ERR_ARG
  # the backward: a desc that the plain entry point accepts, then each defect
  batch, _ = _grad_batch(rng, prm, 33, table, 'relu')
  from test_policy_grad import _Call as GradCall
  bwd = c.lib.sag_policy_backward_norm_device
  gcases = [({}, None, CLIP, ERR_ARG), ({}, tp + 4, CLIP, ERR_ARG), ({}, tp, 0.0, ERR_ARG), ({}, tp, float('nan'), ERR_ARG),
            (dict(flags=2), tp, CLIP, ERR_ARG), (dict(max_blocks=-1), tp, CLIP, ERR_ARG), (dict(pitch=32), tp, CLIP, ERR_ARG),
            (dict(d_adv=None), tp, CLIP, ERR_ARG), (dict(hidden=160), tp, CLIP, ERR_UNSUPPORTED)]
  for change, table_ptr, clip, code in gcases:
    g = GradCall(nat, c, P.pack(prm), batch, 32, 33, 1, G.COEF)
    for f, v in change.items():
      setattr(g.desc, f, v)
    assert bwd(c.h, C.byref(g.desc), table_ptr, clip) == code, (change, table_ptr, clip)
    c.wait()
    assert c.lib.sag_last_error(c.h).decode().startswith('sag_policy_backward_norm_device:')
    assert (g.words() == F32(7.0)).all(), f'{change}: refused, but d_grad was written'
    g.free()
  assert bwd(c.h, None, tp, CLIP) == ERR_ARG and bwd(None, None, tp, CLIP) == ERR_ARG
  # the context is usable afterwards, +inf is a legal clip
  k = _Call(nat, c, P.pack(prm), obs, 32)
  assert fwd(c.h, C.byref(k.desc), tp, float('inf')) == 0
  c.wait()
  assert np.isfinite(k.get('value')[:33]).all()
  k.free(); t.free()


# ----------------------------------------------------------------------------------------------------------------------
# sag.MLPPolicy(normalize_observations=True) and sag.PPOLearner
# ----------------------------------------------------------------------------------------------------------------------
N_ENVS, T = 33, 8
LEARNER = dict(epochs=2, minibatches=3, cost_weight=0.5, ent_coef=0.01, lr=1e-2, std_min=0.5)


def _loop(**kw):
  import safe_adaptation_gym_amd as sag
  from test_reset_loop import _make_env
  env = _make_env('point', 'go_to_goal', n_envs=N_ENVS, seed=3, device_buffers=True, time_limit=5, auto_reset=True)
  env.reset()
  pi = sag.MLPPolicy(env, hidden=32, activation='tanh', seed=1, **kw)
  buf = sag.RolloutBuffer(env, steps=T)
  return sag, env, pi, buf


def _raw_state(pi):
  pi._ctx.wait()
  od = pi.obs_dim
  return pi._ctx.dev_download(pi._obs_state, (1 + 2 * od,), F64), pi._ctx.dev_download(pi._obs_table, (2, od), F32)


@pytest.mark.gpu
def test_policy_owns_running_statistics(nat):
  """33 Point envs, T = 8: the empty state is the identity table (the first collect equals a plain policy's); after
  update_obs_stats(buf) the state is within the tolerance rule of the reference on buf.obs[:T] downloaded and forward() equals
  the plain policy on normalize32; set_obs_norm(get_obs_norm()) reproduces the table's bits; obs_norm_frozen stops the update;
  without the switch the methods raise."""
  sag, env, pi, buf = _loop(normalize_observations=True, obs_clip=5.0)
  od = pi.obs_dim
  state, table = _raw_state(pi)
  assert not state.any() and table.tobytes() == O.table32(O.empty_state(od), 1e-8).tobytes()
  assert pi.get_obs_norm()['count'] == 0 and not pi.obs_norm_frozen
  pi.deterministic = True
  buf.collect(pi)
  buf.wait()
  obs = buf.obs.numpy()
  prm = pi.get_params()
  ident = O.table32(O.empty_state(od), 1e-8)            # under the identity table: the plain network on clamped rows
  mean, v, cv = P.forward_ref32(prm, O.normalize32(obs[0], ident, 5.0), 'tanh')
  assert np.abs(buf.value.numpy()[0] - v).max() <= 1e-5
  pi.update_obs_stats(buf)
  state, table = _raw_state(pi)
  rows = obs[:T].reshape(T * N_ENVS, od)
  _within(state, [rows], 'MLPPolicy.update_obs_stats')
  assert table.tobytes() == O.table32(state, 1e-8).tobytes()
  got = pi.get_obs_norm()
  assert got['count'] == T * N_ENVS and got['mean'].dtype == F64 and (got['mean'] == state[1:1 + od]).all()
  np.testing.assert_array_equal(got['var'], state[1 + od:] / state[0])
  # the forward now reads normalised rows: equal to the plain entry point on normalize32, bit for bit
  c = pi._ctx
  out = _Buf(c, np.full(N_ENVS, SENTINEL, F32))
  pi.forward(buf.obs[2], value=nat.DeviceArray(c, out.p.value, (N_ENVS,), F32))
  c.wait()
  ref = O.normalize32(obs[2], table, 5.0)
  want = _forward(nat, c, prm, ref, 32, activation=1, flags=1)['value'][:N_ENVS]
  np.testing.assert_array_equal(out.get().view(np.uint32), want.view(np.uint32))
  # a second rollout merges; a view [planes, rows, obs_dim] is taken as well as the buffer
  buf.collect(pi)
  buf.wait()
  obs2 = buf.obs.numpy()
  from safe_adaptation_gym_amd.policy import plane_range
  pi.update_obs_stats(plane_range(buf.obs, 0, 3))
  state2, table2 = _raw_state(pi)
  _within(state2, [rows, obs2[:3].reshape(3 * N_ENVS, od)], 'a second batch of three planes')
  # the checkpoint round trip
  pi.set_obs_norm(pi.get_obs_norm())
  state3, table3 = _raw_state(pi)
  assert table3.tobytes() == table2.tobytes() and state3[0] == state2[0] and (state3[1:1 + od] == state2[1:1 + od]).all()
  np.testing.assert_allclose(state3[1 + od:], state2[1 + od:], rtol=4e-16, atol=0)
  pi.set_obs_norm(got['count'], got['mean'], got['var'])
  assert _raw_state(pi)[1].tobytes() == table.tobytes()
  # frozen: nothing moves
  pi.obs_norm_frozen = True
  before = _raw_state(pi)
  pi.update_obs_stats(buf)
  after = _raw_state(pi)
  assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
  out.free()
  with pytest.raises(ValueError):
    pi.set_obs_norm(1.0, np.zeros(od), -np.ones(od))
  with pytest.raises(ValueError):
    sag.MLPPolicy(env, normalize_observations=True, obs_clip=0.0)
  off = sag.MLPPolicy(env, hidden=32)
  assert off._obs_state is None and off._obs_table is None and not off.normalize_observations
  for call in (lambda: off.update_obs_stats(buf), off.get_obs_norm, lambda: off.set_obs_norm(got)):
    with pytest.raises(ValueError):
      call()
  off.close(); pi.close(); buf.close()


@pytest.mark.gpu
def test_learner_update_equals_its_composed_twin(nat):
  """PPOLearner.update() with a normalising policy against a twin composed from the Context methods in the learner's order:
  per round policy_backward_norm then adam, and after the last round obs_stats over buf.obs[0:T].  Parameters, Adam moments,
  the statistics' state and the table match bit for bit; update_obs_stats=False leaves the state alone."""
  from safe_adaptation_gym_amd.policy import plane_range
  sag, env, pi, buf = _loop(normalize_observations=True, obs_clip=5.0)
  c, n, nu, od, N, Pt = pi._ctx, pi.n_params, pi.nu, pi.obs_dim, buf.N, buf.P
  buf.collect(pi)
  pi.update_obs_stats(buf)   # a warm-up rollout: the update below runs under a table that is not the identity
  buf.collect(pi)
  pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  before = pi.get_params()
  state0, table0 = _raw_state(pi)
  assert state0[0] == T * N and (table0[1] != 1).all()
  learner = sag.PPOLearner(pi, buf, **LEARNER)
  assert learner.update_obs_stats
  stats = learner.update(out)
  after = pi.get_params()
  state1, table1 = _raw_state(pi)
  assert state1[0] == 2 * T * N and table1.tobytes() != table0.tobytes()
  _within(state1, [buf.obs.numpy()[:T].reshape(T * N, od)], 'the learner\'s hook', start=state0)
  left = {k: c.dev_download(p, (n,), F32) for k, p in (('m', learner._m), ('v', learner._v))}

  # the twin, on a state, a table and Adam moments of its own
  pi.set_params(before)
  ds, dt = _Buf(c, state0), _Buf(c, np.full((2, od), SENTINEL, F32))
  c.obs_stats(ds.p, dt.p, table_only=True)
  c.wait()
  assert dt.get().tobytes() == table0.tobytes()
  dm, dv = _Buf(c, np.zeros(n, F32)), _Buf(c, np.zeros(n, F32))
  t = 0
  for epoch in range(2):
    for t0, t1 in learner.ranges():
      t += 1
      cut = lambda x: plane_range(x, t0, t1).ptr   # noqa: E731
      c.policy_backward_norm(N, t1 - t0, Pt, 32, pi._buf, cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(out['adv']), cut(out['ret']),
                             pi._gbuf, 1.0 / ((t1 - t0) * N), dt.p, 5.0, d_cadv=cut(out['cadv']), d_cret=cut(out['cret']), clip=0.2,
                             vf_coef=0.5, cvf_coef=0.5, ent_coef=0.01, adv_affine=(1.0, 0.0), cadv_affine=(0.5, 0.0), activation=1)
      c.adam(n, pi._buf, pi._gbuf, dm.p, dv.p, learner.step_size(t), clamp_first=n - nu, clamp_lo=0.5)
  c.obs_stats(ds.p, dt.p, buf.obs.ptr, N, T, Pt, eps=1e-8)
  twin = pi.get_params()
  for k in P.KEYS:
    np.testing.assert_array_equal(twin[k].view(np.uint32), after[k].view(np.uint32), err_msg=f'{k}: update() against its twin')
    assert (after[k] != before[k]).any(), k
  np.testing.assert_array_equal(dm.get().view(np.uint32), left['m'].view(np.uint32))
  np.testing.assert_array_equal(dv.get().view(np.uint32), left['v'].view(np.uint32))
  assert ds.get().tobytes() == state1.tobytes() and dt.get().tobytes() == table1.tobytes()
  assert set(stats) == {'policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl', 'clip_fraction'}
  # a plain policy under the same parameters takes another step: the normalisation is inside the backward pass
  plain = sag.MLPPolicy(env, hidden=32, activation='tanh', seed=1)
  plain.set_params(before)
  pl = sag.PPOLearner(plain, buf, **LEARNER)
  pl.update(out)
  assert any((plain.get_params()[k] != after[k]).any() for k in ('W1', 'W2'))
  pl.close(); plain.close()
  # the hook switched off, and the hook under a frozen policy
  quiet = sag.PPOLearner(pi, buf, update_obs_stats=False, **LEARNER)
  quiet.update(out)
  assert _raw_state(pi)[0].tobytes() == state1.tobytes()
  quiet.close()
  pi.obs_norm_frozen = True
  learner.update(out)
  assert _raw_state(pi)[0].tobytes() == state1.tobytes()
  for b in (ds, dt, dm, dv):
    b.free()
  learner.close(); pi.close(); buf.close()

"""sag_policy_backward_rows_device (the ROWS instances of csrc/sag_policy_grad.hpp): the backward pass over a list of rows
gathered in place, against policy_grad_ref's float64 gradient evaluated on batch[k][rows] - never against the kernel.

The tolerance is test_policy_grad.py's rule, not a new constant: per case 8 times the error of the reference's own float32
restatement against its float64 one, on the rows of the list.  The planes are 3 x 33 and 3 x 130 rows at a pitch rounded up to
64 with NaN in every pad row and in 4 pad columns per observation row, so a source row computed wrongly reads a NaN.  Lists:
one entry, one full tile, a tile plus one, three tiles and a ragged last (97), a full permutation, duplicates, and entries
outside the planes among valid ones - those rows are absent: the result is the reference over the valid entries and statistic 5
their count.  The identity list must give the bits of the contiguous entry points.  The cases at hidden <= 96 and lists of
<= 97 entries also run on the host build of the device sources (test_shuffle_hostemu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import obs_norm_ref as N
import policy_grad_ref as G
import policy_ref as P
from test_device_reset import KEY
from test_policy_grad import ACCUMULATE, ERR_ARG, ERR_UNSUPPORTED, F32, GUARD, ROBOTS, SENTINEL, _Call, _check, _reference, _setup

HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
OBS_PAD = 4
OBS_CLIP = 5.0
INT_MIN, INT_MAX = -2**31, 2**31 - 1


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
      made[robot] = nat.Context(robot, 8, seed=KEY)
    return made[robot]
  yield get
  for c in made.values():
    c.close()


class _Rows(_Call):
  """test_policy_grad._Call plus a device row list (and a table): run() is sag_policy_backward_rows_device, contiguous() the
  entry point the list-free call of the same desc goes to."""

  def __init__(self, nat, c, prm, batch, hidden, n_rows, n_planes, coef, rows, activation='relu', table=None, **kw):
    super().__init__(nat, c, prm, batch, hidden, n_rows, n_planes, coef, activation, obs_pad=OBS_PAD, **kw)
    self.rows = np.ascontiguousarray(rows, np.int32)
    self.p['rows'] = c.dev_alloc(self.rows.nbytes + 4)
    c.dev_upload(self.p['rows'], self.rows)
    self.table = None
    if table is not None:
      self.table = self.p['table'] = c.dev_alloc(table.nbytes)
      c.dev_upload(self.table, np.ascontiguousarray(table, F32))

  def raw(self, d_rows, n_index, d_table, obs_clip):
    rc = self.c.lib.sag_policy_backward_rows_device(self.c.h, C.byref(self.desc), d_rows, n_index, d_table, obs_clip)
    self.c.wait()
    return rc

  def run(self):
    return self.raw(self.p['rows'].value, len(self.rows), self.table.value if self.table else None, OBS_CLIP if self.table else 0.0)

  def contiguous(self):
    if self.table:
      rc = self.c.lib.sag_policy_backward_norm_device(self.c.h, C.byref(self.desc), self.table.value, OBS_CLIP)
    else:
      rc = self.c.lib.sag_policy_backward_device(self.c.h, C.byref(self.desc))
    self.c.wait()
    return rc

  def list_unchanged(self):
    return self.c.dev_download(self.p['rows'], self.rows.shape, np.int32).tobytes() == self.rows.tobytes()


def _list(kind, total, rng):
  """-> the list (int32).  Entries outside [0, total) are absent rows."""
  if kind == 'one':
    return np.array([total - 1], np.int32)        # the last row of the last plane
  if kind == 'tile':
    return rng.choice(total, 32, replace=False).astype(np.int32)
  if kind == 'tile+1':
    return rng.choice(total, 33, replace=False).astype(np.int32)
  if kind == '97':
    return rng.choice(total, 97, replace=False).astype(np.int32)
  if kind == 'perm':
    return rng.permutation(total).astype(np.int32)
  if kind == 'dups':                              # 50 draws with replacement, and one row five times in one tile
    r = rng.randint(0, total, 50)
    r[[3, 4, 9, 20, 31]] = r[0]
    return r.astype(np.int32)
  assert kind == 'absent'                         # 45 entries, 9 of them outside the planes, in both tiles and at both ends
  r = rng.choice(total, 45, replace=False).astype(np.int64)
  r[[0, 5, 6, 31, 32, 40, 44]] = [-1, total, INT_MAX, INT_MIN, total + 1, -total, total]
  r[[17, 18]] = [-1, total * 2]
  return r.astype(np.int32)


def _sub(batch, rows, total, cost):
  valid = rows[(rows >= 0) & (rows < total)]
  sub = {k: v[valid] for k, v in batch.items()}
  if not cost:
    sub['cadv'] = sub['cret'] = None
  return sub, len(valid)


# (robot, hidden, activation, rows per plane, list, cost channel): every value of each axis, every list on both geometries' kind
CASES = [('point', 32, 'relu', 33, 'one', True), ('point', 32, 'relu', 33, 'tile', True), ('point', 64, 'tanh', 33, 'tile+1', False),
         ('point', 96, 'relu', 130, '97', True), ('doggo', 32, 'tanh', 33, 'perm', True), ('doggo', 96, 'relu', 33, 'dups', False),
         ('doggo', 32, 'relu', 130, 'absent', True), ('point', 64, 'relu', 33, 'absent', False), ('point', 32, 'tanh', 130, 'dups', True),
         ('doggo', 64, 'relu', 130, 'tile+1', True), ('doggo', 96, 'tanh', 130, 'one', False)] + (
             [] if HOSTEMU else [('point', 128, 'relu', 130, 'perm', True), ('doggo', 128, 'tanh', 130, '97', True),
                                 ('doggo', 128, 'relu', 33, 'absent', False)])


@pytest.mark.gpu
@pytest.mark.parametrize('robot,hidden,activation,n_rows,kind,cost', CASES)
def test_gathered_gradient_against_the_float64_reference_on_the_listed_rows(nat, ctxs, robot, hidden, activation, n_rows, kind, cost):
  c = ctxs(robot)
  total = 3 * n_rows
  prm, batch, shapes = _setup(robot, hidden, total, activation, seed=7000 + hidden + n_rows)
  rows = _list(kind, total, np.random.RandomState(hidden + n_rows))
  sub, n_valid = _sub(batch, rows, total, cost)
  assert n_valid == len(rows) - (9 if kind == 'absent' else 0)
  coef = dict(G.COEF, scale=1.0 / len(rows))
  ref, tol, _ = _reference(prm, sub, coef, activation)
  k = _Rows(nat, c, P.pack(prm), batch, hidden, n_rows, 3, coef, rows, activation, drop=() if cost else ('cadv', 'cret'))
  assert k.pitch % 64 == 0 and k.pitch > n_rows and np.isnan(k.host['obs'][:, n_rows:]).all() and np.isnan(k.host['obs'][:, :, -OBS_PAD:]).all()
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  _check(k.grad(), shapes, ref, tol, f'{robot} {hidden} {activation} 3x{n_rows} {kind} cost={cost}')
  # under scale = 1 statistics 4 and 5 are sums of ones: the rows that took part, and the clipped ones among them, exactly
  k.desc.scale = 1.0
  k.fill(SENTINEL)
  assert k.run() == 0
  s = k.grad()[-8:]
  assert s[5] == n_valid and s[4] == round(float(ref[1][4]) * len(rows)), (s, n_valid)
  if not cost:
    assert s[2] == 0
  assert k.inputs_unchanged() and k.list_unchanged()
  k.free()


@pytest.mark.gpu
@pytest.mark.parametrize('robot,hidden,activation,n_rows,normalised', [('point', 32, 'relu', 33, False), ('doggo', 32, 'tanh', 33, True)] + (
    [] if HOSTEMU else [('doggo', 96, 'tanh', 130, False), ('point', 64, 'relu', 130, True)]))   # (390 rows x 8 calls: the host build's minute)
def test_the_identity_list_gives_the_bits_of_the_contiguous_call(nat, ctxs, robot, hidden, activation, n_rows, normalised):
  """0, 1, ..., n_planes * n_rows - 1: the same tiles in the same blocks and the same reduce - equal words, with one tile per
  block and with several (max_blocks = 2), replacing and accumulating; with a table against sag_policy_backward_norm_device."""
  c = ctxs(robot)
  od, _ = ROBOTS[robot]
  total = 3 * n_rows
  rng = np.random.RandomState(99 + n_rows)
  prm, batch, shapes = _setup(robot, hidden, total, activation, seed=7100 + n_rows)
  table = np.stack([rng.uniform(-0.5, 0.5, od), rng.uniform(0.5, 2.0, od)]).astype(F32) if normalised else None
  coef = dict(G.COEF, scale=1.0 / total)
  for max_blocks in (0, 2):
    k = _Rows(nat, c, P.pack(prm), batch, hidden, n_rows, 3, coef, np.arange(total), activation, table=table, max_blocks=max_blocks)
    for flags, fill in ((0, SENTINEL), (ACCUMULATE, 0.25)):
      k.desc.flags = flags
      k.fill(fill)
      assert k.contiguous() == 0, c.lib.sag_last_error(c.h)
      want = k.words()
      k.fill(fill)
      assert k.run() == 0, c.lib.sag_last_error(c.h)
      got = k.words()
      assert np.isfinite(got).all() and (got[k.n_words:] == F32(fill)).all()
      np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f'max_blocks {max_blocks} flags {flags}')
    k.free()


@pytest.mark.gpu
def test_a_shuffled_list_under_a_table_equals_the_raw_rows_call_on_normalize32(nat, ctxs):
  """The table and the list together (Point, hidden 32, 3 x 33 rows, a permutation with two absent entries): all words equal
  the table-free rows call on observations normalised on the host, bit for bit - and that call is within tolerance of the
  float64 reference on the normalised rows."""
  c = ctxs('point')
  od, _ = ROBOTS['point']
  rng = np.random.RandomState(5)
  prm, batch, shapes = _setup('point', 32, 99, 'relu', seed=7200)
  table = np.stack([rng.uniform(-0.5, 0.5, od), rng.uniform(0.5, 4.0, od)]).astype(F32)   # |x - mean| rstd reaches 8: clamped at 5
  rows = rng.permutation(99).astype(np.int32)
  rows[[2, 70]] = [99, -1]
  coef = dict(G.COEF, scale=1.0 / 99)
  k = _Rows(nat, c, P.pack(prm), batch, 32, 33, 3, coef, rows, table=table)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  got = k.grad()
  k.free()
  plain = dict(batch, obs=N.normalize32(batch['obs'], table, OBS_CLIP))
  assert (np.abs(plain['obs']) == F32(OBS_CLIP)).any(), 'the clamp was not exercised'
  k = _Rows(nat, c, P.pack(prm), plain, 32, 33, 3, coef, rows)
  assert k.run() == 0, c.lib.sag_last_error(c.h)
  want = k.grad()
  k.free()
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  sub, n_valid = _sub(plain, rows, 99, True)
  ref, tol, _ = _reference(prm, sub, coef, 'relu')
  _check(got, shapes, ref, tol, 'table and list')
  assert n_valid == 97


@pytest.mark.gpu
def test_accumulate_adds_the_second_half_of_a_permutation(nat, ctxs):
  """Two minibatches of one permutation, the second accumulated onto the first under scale = 1 / n: the whole batch's mean."""
  c = ctxs('point')
  total = 99
  prm, batch, shapes = _setup('point', 64, total, 'tanh', seed=7300)
  rows = np.random.RandomState(8).permutation(total).astype(np.int32)
  coef = dict(G.COEF, scale=1.0 / total)
  ref, tol, _ = _reference(prm, batch, coef, 'tanh')
  k = _Rows(nat, c, P.pack(prm), batch, 64, 33, 3, coef, rows, 'tanh')
  assert k.raw(k.p['rows'].value, 49, None, 0.0) == 0, c.lib.sag_last_error(c.h)
  first = k.grad()
  assert abs(first[-3] - 49 / 99) < 1e-6
  k.desc.flags = ACCUMULATE
  assert k.raw(k.p['rows'].value + 4 * 49, 50, None, 0.0) == 0, c.lib.sag_last_error(c.h)
  _check(k.grad(), shapes, ref, tol, 'entries 0 ... 48, then 49 ... 98 on top')
  assert k.inputs_unchanged() and k.list_unchanged()
  k.free()


@pytest.mark.gpu
def test_refusals_enqueue_nothing(nat, ctxs):
  c = ctxs('point')
  od, _ = ROBOTS['point']
  prm, batch, shapes = _setup('point', 32, 33, 'relu', seed=7400)
  table = np.stack([np.zeros(od), np.ones(od)]).astype(F32)
  k = _Rows(nat, c, P.pack(prm), batch, 32, 33, 1, dict(G.COEF, scale=1.0 / 33), np.arange(33), table=table)
  good = {f: getattr(k.desc, f) for f, _ in k.desc._fields_}
  rp, tp = k.p['rows'].value, k.table.value

  def refused(code=ERR_ARG, d_rows=rp, n_index=33, d_table=None, obs_clip=0.0, **change):
    for f, v in good.items():
      setattr(k.desc, f, v)
    for f, v in change.items():
      setattr(k.desc, f, v)
    rc = k.raw(d_rows, n_index, d_table, obs_clip)
    assert rc == code, (change, d_rows, n_index, d_table, obs_clip, rc)
    assert (k.words() == F32(SENTINEL)).all(), f'{change}: d_grad was written'
    assert c.lib.sag_last_error(c.h).decode().startswith('sag_policy_backward_rows_device:')

  # the list
  refused(d_rows=None)
  refused(d_rows=rp + 2)
  refused(n_index=0)
  refused(n_index=-33)
  # the table and its clip (without a table the clip is ignored, whatever it is)
  refused(d_table=tp + 4, obs_clip=OBS_CLIP)
  for clip in (0.0, -1.0, float('nan'), float('inf')):
    refused(d_table=tp, obs_clip=clip)
  # everything the contiguous calls refuse
  for f in ('d_params', 'd_obs', 'd_actions', 'd_logp_old', 'd_adv', 'd_ret', 'd_grad'):
    refused(**{f: None})
  refused(d_obs=good['d_obs'] + 4)
  for f in ('d_params', 'd_actions', 'd_logp_old', 'd_adv', 'd_ret', 'd_cadv', 'd_cret', 'd_grad'):
    refused(**{f: good[f] + 2})
  for h in (0, 16, 48, 288, -32):
    refused(hidden=h)
  for h in (160, 192, 224, 256):
    refused(ERR_UNSUPPORTED, hidden=h)
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
  f = c.lib.sag_policy_backward_rows_device
  assert f(c.h, None, rp, 33, None, 0.0) == ERR_ARG and f(None, None, rp, 33, None, 0.0) == ERR_ARG
  # the context is usable afterwards; without a table a NaN clip is ignored
  for name, v in good.items():
    setattr(k.desc, name, v)
  assert k.raw(rp, 33, None, float('nan')) == 0
  assert np.isfinite(k.grad()).all()
  assert k.inputs_unchanged() and k.list_unchanged()
  k.free()

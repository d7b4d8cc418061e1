"""The rollout buffer: sag_append_rows_device and sag_gae_device (csrc/sag_buffer.hpp) against the NumPy restatements of
tests/rollout_ref.py, then sag.RolloutBuffer against the loop written by hand - env.step(sync=True) of a twin env with
final_observation=True and every return downloaded.  Two paths through the same step, tracker and reset kernels on the same
device, and a GAE recipe in which every operation is rounded on its own: every comparison is exact.

The kernel cases (append, GAE) also run on the host build of the device sources: test_rollout_buffer_hostemu.py."""
import ctypes as C

import numpy as np
import pytest

import rollout_ref as R
from test_device_reset import KEY
from test_final_obs import MASKS, _sentinel
from test_reset_loop import _make_env, _np

ERR_ARG = -1   # SAG_ERR_ARG
N = 130        # two full wavefronts and a partial one of two lanes
PITCH = 256
DEPTH = 8      # GAE_DEPTH of csrc/sag_buffer.hpp: T = 7, 8, 9 are depth - 1, depth, depth + 1
PAIRS = [(0.99, 0.95), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)]
OUT_FILL = 0x7fc12345   # a NaN no arithmetic produces: the bits an untouched output element keeps


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(nat):
  c = nat.Context('point', N, seed=KEY)
  yield c
  c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 0. the reference itself (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _random_channel(rng, T, n, p_end=0.05):
  reward = rng.normal(0, 1, (T, n)).astype(np.float32)
  value = rng.normal(0, 3, (T + 1, n)).astype(np.float32)
  ended = np.where(rng.rand(T, n) < p_end, rng.randint(1, 3, (T, n)), 0).astype(np.uint8)
  return reward, value, ended


def test_fp32_recipe_against_the_textbook_recurrence_in_fp64():
  """gae_ref32 (the kernel's recipe) against gae_ref64 on 10 000 random trajectories of T = 64, truncations bootstrapped from
  random final values: the largest deviation of advantages and returns stays below 64 * 2^-23 * max(1, max |ret64|) - 64
  steps, each a handful of roundings of relative size 2^-24 on numbers no larger than the largest return.  A check of the
  reference, not of the kernel.  The 10 000 run side by side (gae_ref32_batch), which is first shown to equal the scalar
  recipe bit for bit."""
  rng = np.random.RandomState(64)
  T, n = 64, 10000
  reward, value, ended = _random_channel(rng, T, n)
  cost = (rng.rand(T, n) < 0.2).astype(np.uint8)
  k = int((ended == 2).sum())
  slot = np.full((T, n), -1, np.int32)
  slot[ended == 2] = rng.permutation(k)
  final = rng.normal(0, 3, k).astype(np.float32)
  boot = np.zeros((T, n), np.float32)
  boot[ended == 2] = final[slot[ended == 2]]
  sub = slice(0, 200)
  for is_cost, (g, l) in ((False, (0.99, 0.95)), (True, (0.995, 0.9)), (False, (1.0, 1.0))):
    a32, r32 = R.gae_ref32_batch(reward, cost, ended, value, g, l, slot, final, k, is_cost=is_cost)
    s32 = R.gae_ref32(reward[:, sub], cost[:, sub], ended[:, sub], value[:, sub], g, l, slot[:, sub], final, k, is_cost=is_cost)
    np.testing.assert_array_equal(a32[:, sub].view(np.uint32), s32[0].view(np.uint32))
    np.testing.assert_array_equal(r32[:, sub].view(np.uint32), s32[1].view(np.uint32))
    r = (cost != 0).astype(np.float64) if is_cost else reward
    a64, r64 = R.gae_ref64(r, ended, value, float(np.float32(g)), float(np.float32(l)), boot)
    bound = 64 * 2.0**-23 * max(1.0, np.abs(r64).max())
    dev = max(np.abs(a32 - a64).max(), np.abs(r32 - r64).max())
    print(f'cost channel {is_cost}, gamma {g}, lam {l}: largest deviation {dev:.3e}, bound {bound:.3e}, max |ret64| {np.abs(r64).max():.3f}')
    assert dev < bound


# ---------------------------------------------------------------------------------------------------------------------
# 1. sag_append_rows_device
# ---------------------------------------------------------------------------------------------------------------------
class _Append:
  """Device buffers of one append configuration and the call itself."""

  def __init__(self, ctx, row_bytes, capacity, src):
    self.c, self.rb, self.cap = ctx, row_bytes, capacity
    self.fill = _sentinel((capacity, row_bytes))
    self.b = {k: ctx.dev_alloc(s) for k, s in (('src', src.nbytes + 16), ('store', capacity * row_bytes + 16), ('mask', N),
                                                ('count', 16), ('slot', 4 * N + 16))}
    ctx.dev_upload(self.b['src'], src)
    self.set_count(0)

  def set_count(self, c0):
    self.c.dev_upload(self.b['count'], np.array([c0], np.int32))

  def refill(self):
    self.c.dev_upload(self.b['store'], self.fill)
    self.c.dev_upload(self.b['slot'], np.full(N, -7, np.int32))

  def call(self, m8, restart=0):
    self.c.dev_upload(self.b['mask'], m8)
    b = self.b
    self.c.append_rows(b['mask'], self.rb, b['src'], b['store'], self.cap, b['count'], restart, b['slot'])
    self.c.wait()
    return self.read()

  def read(self):
    c, b = self.c, self.b
    return (c.dev_download(b['store'], (self.cap, self.rb), np.uint8), c.dev_download(b['slot'], (N,), np.int32),
            int(c.dev_download(b['count'], (1,), np.int32)[0]))

  def free(self):
    for p in self.b.values():
      self.c.dev_free(p)


@pytest.mark.gpu
@pytest.mark.parametrize('row_bytes', [16, 240], ids=['1 piece', '15 pieces'])
def test_append_rows_under_every_mask(ctx, row_bytes):
  """Rows of 16 B and 240 B of random bytes into a store of sentinel bytes, under every mask of test_final_obs.MASKS but NULL,
  from a counter that starts at 0 and at 5: the slots of the set envs are exactly {c0 ... c0 + k - 1}, ascending with the env
  index inside each aligned group of 64, store[slot[i]] == src[i], unclaimed rows still sentinel, -1 elsewhere, the source
  unchanged (rollout_ref.append_ref)."""
  rng = np.random.RandomState(row_bytes)
  src = rng.randint(0, 256, (N, row_bytes)).astype(np.uint8)
  a = _Append(ctx, row_bytes, N + 8, src)
  for name, kind in MASKS.items():
    if kind is None:
      continue
    m8 = kind(N, rng, None)
    for c0 in (0, 5):
      a.refill()
      a.set_count(c0)
      store, slot, count = a.call(m8)
      assert R.append_ref(m8, src, a.fill, a.cap, c0, store, slot, count) == (m8 != 0).sum(), name
      np.testing.assert_array_equal(ctx.dev_download(a.b['src'], src.shape, np.uint8), src, err_msg=f'mask {name}: the source')
  a.free()


@pytest.mark.gpu
def test_append_rows_accumulates_and_restarts(ctx):
  """Two calls without restart accumulate the count and fill consecutive slots; restart zeroes the count first."""
  rng = np.random.RandomState(3)
  src = rng.randint(0, 256, (N, 48)).astype(np.uint8)
  a = _Append(ctx, 48, 2 * N, src)
  m1, m2 = MASKS['random 30 %'](N, rng, None), MASKS['bytes 2 and 255'](N, rng, None)
  k1, k2 = int((m1 != 0).sum()), int((m2 != 0).sum())
  a.refill()
  store1, slot1, count1 = a.call(m1)
  assert R.append_ref(m1, src, a.fill, a.cap, 0, store1, slot1, count1) == k1
  store2, slot2, count2 = a.call(m2)
  assert count2 == k1 + k2
  assert R.append_ref(m2, src, store1, a.cap, k1, store2, slot2, count2) == k2   # (the rows of the first call are `fill` here: kept)
  store3, slot3, count3 = a.call(m1, restart=1)
  assert count3 == k1
  assert R.append_ref(m1, src, store2, a.cap, 0, store3, slot3, count3) == k1
  store4, slot4, count4 = a.call(np.zeros(N, np.uint8), restart=1)
  assert count4 == 0 and (slot4 == -1).all()
  np.testing.assert_array_equal(store4, store3)
  a.free()


@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 9])
def test_append_rows_into_a_store_that_is_too_small(ctx, c0):
  """capacity 50 under a full mask (and from a counter at 9): exactly capacity - c0 rows are written, each matches its env
  through d_slot, the rest get -1, the count is c0 + k; a second call into the full store writes nothing and counts on."""
  rng = np.random.RandomState(4)
  src = rng.randint(0, 256, (N, 240)).astype(np.uint8)
  a = _Append(ctx, 240, 50, src)
  a.refill()
  a.set_count(c0)
  ones = np.ones(N, np.uint8)
  store, slot, count = a.call(ones)
  assert R.append_ref(ones, src, a.fill, 50, c0, store, slot, count) == 50 - c0
  assert count == c0 + N and (slot >= 0).sum() == 50 - c0 and (slot[slot < 0] == -1).all()
  store2, slot2, count2 = a.call(MASKS['random 30 %'](N, rng, None))
  assert count2 > count and (slot2 == -1).all()
  np.testing.assert_array_equal(store2, store)
  a.free()


@pytest.mark.gpu
def test_append_rows_refuses_bad_arguments(nat, ctx):
  """Every refusal of the header comment returns SAG_ERR_ARG and leaves store, slots and count as they were."""
  rb = 48
  src = np.random.RandomState(5).randint(0, 256, (N, rb)).astype(np.uint8)
  a = _Append(ctx, rb, N, src)
  b = {k: p.value for k, p in a.b.items()}
  assert all(v % 16 == 0 for v in b.values())
  ok = dict(mask=b['mask'], rb=rb, src=b['src'], store=b['store'], cap=N, count=b['count'], slot=b['slot'])
  bad = {'NULL d_mask': dict(mask=None), 'NULL d_src': dict(src=None), 'NULL d_store': dict(store=None), 'NULL d_count': dict(count=None),
         'NULL d_slot': dict(slot=None), 'row_bytes 0': dict(rb=0), 'row_bytes -16': dict(rb=-16), 'row_bytes 40': dict(rb=40),
         'row_bytes 8': dict(rb=8), 'd_src + 4': dict(src=b['src'] + 4), 'd_store + 8': dict(store=b['store'] + 8),
         'd_src == d_store': dict(src=b['store']), 'capacity 0': dict(cap=0), 'capacity -3': dict(cap=-3),
         'd_count + 2': dict(count=b['count'] + 2), 'd_slot + 1': dict(slot=b['slot'] + 1)}
  ctx.dev_upload(a.b['mask'], np.ones(N, np.uint8))
  for what, change in bad.items():
    k = dict(ok, **change)
    for restart in (0, 1):
      a.refill()
      a.set_count(11)
      rc = ctx.lib.sag_append_rows_device(ctx.h, k['mask'], k['rb'], k['src'], k['store'], k['cap'], k['count'], restart, k['slot'])
      ctx.wait()
      assert rc == ERR_ARG, f'{what}: {rc}'
      store, slot, count = a.read()
      np.testing.assert_array_equal(store, a.fill, err_msg=f'{what}: the store was written')
      assert (slot == -7).all() and count == 11, what
  with pytest.raises(nat.SagError):
    ctx.append_rows(a.b['mask'], 40, a.b['src'], a.b['store'], N, a.b['count'], 0, a.b['slot'])
  a.refill()
  store, slot, count = a.call(np.ones(N, np.uint8), restart=1)   # the context is usable after the refusals
  assert R.append_ref(np.ones(N, np.uint8), src, a.fill, N, 0, store, slot, count) == N
  a.free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sag_gae_device
# ---------------------------------------------------------------------------------------------------------------------
def _pitched(a, pad):
  """[rows, N, ...] -> [rows, PITCH, ...] with the pad columns set to `pad`."""
  out = np.full((a.shape[0], PITCH) + a.shape[2:], pad, a.dtype)
  out[:, :N] = a
  return out


def _patterns(rng, T):
  """name -> (ended [T, N] u8, slot [T, N] int32 or None (NULL d_slot), capacity, final values given)"""
  def finals(ended, frac_lost=0.0):
    k = int((ended == 2).sum())
    cap = k + 3
    slot = np.full((T, N), -1, np.int32)
    s = rng.permutation(k).astype(np.int32)
    lost = rng.rand(k) < frac_lost
    s[lost] = np.where(rng.rand(int(lost.sum())) < 0.5, -1, cap)   # not kept: -1, or a slot past the capacity
    slot[ended == 2] = s
    return slot, cap
  none = np.zeros((T, N), np.uint8)
  ends = none.copy()
  ends[0], ends[T - 1] = 1, 1
  trunc = (rng.rand(T, N) < 0.2).astype(np.uint8) * 2
  trunc[T - 1, :5] = 2
  mix = np.where(rng.rand(T, N) < 0.05, rng.randint(1, 3, (T, N)), 0).astype(np.uint8)
  mix[T // 2, 0], mix[T // 2, 1] = 1, 2
  s_trunc, c_trunc = finals(trunc)
  s_mix, c_mix = finals(mix, 0.3)
  return {'none': (none, np.full((T, N), -1, np.int32), 1, True),
          'terminated at both ends': (ends, np.full((T, N), -1, np.int32), 1, True),
          'truncations with slots': (trunc, s_trunc, c_trunc, True),
          'truncations whose slot is -1': (trunc, np.full((T, N), -1, np.int32), c_trunc, True),
          'NULL d_slot': (trunc, None, c_trunc, True),
          'slots without final values': (trunc, s_trunc, c_trunc, False),
          'random 5 % mix': (mix, s_mix, c_mix, True)}


class _Gae:
  """Device arrays of one T, pitched to 256 with poisoned pad columns, and the call."""
  KEYS = ('reward', 'cost', 'ended', 'value', 'cvalue', 'slot', 'fv', 'fcv', 'adv', 'ret', 'cadv', 'cret')

  def __init__(self, ctx, T, cap_max):
    self.c, self.T = ctx, T
    P = PITCH
    sizes = dict(reward=T * P * 8, cost=T * P, ended=T * P, value=(T + 1) * P * 4, cvalue=(T + 1) * P * 4, slot=T * P * 4,
                 fv=cap_max * 4, fcv=cap_max * 4, adv=T * P * 4, ret=T * P * 4, cadv=T * P * 4, cret=T * P * 4)
    self.b = {k: ctx.dev_alloc(s + 16) for k, s in sizes.items()}
    self.host = {}

  def upload(self, **arrays):
    for k, a in arrays.items():
      self.host[k] = np.ascontiguousarray(a)
      self.c.dev_upload(self.b[k], self.host[k])

  def clear_outputs(self):
    for k in ('adv', 'ret', 'cadv', 'cret'):
      self.c.dev_upload(self.b[k], np.full((self.T, PITCH), OUT_FILL, np.uint32))

  def desc(self, nat, g, l, cg, cl, cap, cost=True, slot=True, finals=True, **change):
    b = {k: p.value for k, p in self.b.items()}
    d = dict(T=self.T, pitch=PITCH, capacity=cap, gamma=g, lam=l, cost_gamma=cg, cost_lam=cl, d_reward=b['reward'], d_cost=b['cost'],
             d_ended=b['ended'], d_value=b['value'], d_cvalue=b['cvalue'] if cost else None, d_slot=b['slot'] if slot else None,
             d_final_value=b['fv'] if finals else None, d_final_cvalue=b['fcv'] if finals and cost else None, d_adv=b['adv'],
             d_ret=b['ret'], d_cadv=b['cadv'] if cost else None, d_cret=b['cret'] if cost else None)
    d.update(change)
    return nat.GaeDesc(**d)

  def outputs(self):
    return {k: self.c.dev_download(self.b[k], (self.T, PITCH), np.uint32) for k in ('adv', 'ret', 'cadv', 'cret')}

  def inputs_unchanged(self, what):
    for k, h in self.host.items():
      np.testing.assert_array_equal(self.c.dev_download(self.b[k], h.shape, h.dtype).view(np.uint8), h.view(np.uint8),
                                    err_msg=f'{what}: input {k} changed')

  def free(self):
    for p in self.b.values():
      self.c.dev_free(p)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 37])
def test_gae_equals_the_fp32_recipe_bit_for_bit(nat, ctx, T):
  """130 envs at pitch 256, the pad columns NaN (values, rewards), ended = 7 and cost = 1: T around the pipeline depth and
  several passes of it; every ended pattern; with and without the cost channel; four (gamma, lam) pairs and a different pair
  for the cost channel.  adv, ret, cadv, cret equal gae_ref32 bit for bit, the output pad columns keep their fill, the inputs
  are unchanged."""
  rng = np.random.RandomState(100 + T)
  reward = rng.normal(0, 1, (T, N, 2)).astype(np.float32)
  cost = (rng.rand(T, N) < 0.3).astype(np.uint8) * rng.randint(1, 256, (T, N)).astype(np.uint8)
  value = rng.normal(0, 3, (T + 1, N)).astype(np.float32)
  cvalue = rng.normal(2, 2, (T + 1, N)).astype(np.float32)
  pats = _patterns(rng, T)
  cap_max = max(p[2] for p in pats.values())
  fv, fcv = rng.normal(0, 3, cap_max).astype(np.float32), rng.normal(2, 2, cap_max).astype(np.float32)
  g = _Gae(ctx, T, cap_max)
  g.upload(reward=_pitched(reward, np.nan), cost=_pitched(cost, 1), value=_pitched(value, np.nan), cvalue=_pitched(cvalue, np.nan), fv=fv, fcv=fcv)
  for name, (ended, slot, cap, finals) in pats.items():
    g.upload(ended=_pitched(ended, 7), slot=_pitched(slot if slot is not None else np.zeros((T, N), np.int32), -1))
    for j, (gm, lm) in enumerate(PAIRS):
      cg, cl = PAIRS[(j + 1) % len(PAIRS)]
      ref_slot, ref_fv, ref_fcv = (slot, fv, fcv) if finals else (None, None, None)
      want = dict(zip(('adv', 'ret'), R.gae_ref32(reward[..., 0], cost, ended, value, gm, lm, ref_slot, ref_fv, cap)))
      want.update(zip(('cadv', 'cret'), R.gae_ref32(None, cost, ended, cvalue, cg, cl, ref_slot, ref_fcv, cap, is_cost=True)))
      for with_cost in (True, False):
        what = f'T {T}, {name}, gamma {gm}, lam {lm}, cost channel {with_cost}'
        g.clear_outputs()
        d = g.desc(nat, gm, lm, cg, cl, cap, cost=with_cost, slot=slot is not None, finals=finals)
        rc = ctx.lib.sag_gae_device(ctx.h, C.byref(d))
        ctx.wait()
        assert rc == 0, f'{what}: {rc} {ctx.lib.sag_last_error(ctx.h)}'
        out = g.outputs()
        for k, o in out.items():
          if k in ('cadv', 'cret') and not with_cost:
            assert (o == OUT_FILL).all(), f'{what}: {k} was written'
            continue
          np.testing.assert_array_equal(o[:, :N], want[k].view(np.uint32), err_msg=f'{what}: {k}')
          assert (o[:, N:] == OUT_FILL).all(), f'{what}: pad columns of {k} were written'
    g.inputs_unchanged(f'T {T}, {name}')
  g.free()


@pytest.mark.gpu
def test_gae_through_the_wrapper(nat, ctx):
  """Context.gae() fills the descriptor: cost_gamma / cost_lam default to gamma / lam."""
  T = 5
  rng = np.random.RandomState(7)
  reward, value, ended = _random_channel(rng, T, N, 0.1)
  cost = (rng.rand(T, N) < 0.3).astype(np.uint8)
  g = _Gae(ctx, T, 4)
  r2 = np.stack([reward, np.full_like(reward, np.nan)], -1)
  g.upload(reward=_pitched(r2, np.nan), cost=_pitched(cost, 1), value=_pitched(value, np.nan), cvalue=_pitched(value, np.nan),
           ended=_pitched(ended, 7))
  g.clear_outputs()
  b = g.b
  ctx.gae(T, PITCH, b['reward'], b['cost'], b['ended'], b['value'], b['adv'], b['ret'], 0.9, 0.8, d_cvalue=b['cvalue'], d_cadv=b['cadv'],
          d_cret=b['cret'])
  ctx.wait()
  out = g.outputs()
  want = R.gae_ref32(reward, cost, ended, value, 0.9, 0.8) + R.gae_ref32(None, cost, ended, value, 0.9, 0.8, is_cost=True)
  for k, w in zip(('adv', 'ret', 'cadv', 'cret'), want):
    np.testing.assert_array_equal(out[k][:, :N], w.view(np.uint32), err_msg=k)
  with pytest.raises(nat.SagError):
    ctx.gae(T, PITCH, b['reward'], b['cost'], b['ended'], b['value'], b['adv'], b['ret'], 1.5, 0.8)
  g.free()


@pytest.mark.gpu
def test_gae_refuses_bad_arguments(nat, ctx):
  """Every refusal of the header comment returns SAG_ERR_ARG, and the outputs are untouched."""
  T = 3
  rng = np.random.RandomState(8)
  g = _Gae(ctx, T, 8)
  g.upload(reward=np.zeros((T, PITCH, 2), np.float32), cost=np.zeros((T, PITCH), np.uint8), ended=np.zeros((T, PITCH), np.uint8),
           value=rng.normal(0, 1, (T + 1, PITCH)).astype(np.float32), cvalue=rng.normal(0, 1, (T + 1, PITCH)).astype(np.float32),
           slot=np.full((T, PITCH), -1, np.int32), fv=np.zeros(8, np.float32), fcv=np.zeros(8, np.float32))
  b = {k: p.value for k, p in g.b.items()}
  nan, inf = float('nan'), float('inf')
  bad = {'T 0': dict(T=0), 'T -1': dict(T=-1), 'pitch < n_envs': dict(pitch=N - 1), 'NULL d_reward': dict(d_reward=None),
         'NULL d_cost': dict(d_cost=None), 'NULL d_ended': dict(d_ended=None), 'NULL d_value': dict(d_value=None),
         'NULL d_adv': dict(d_adv=None), 'NULL d_ret': dict(d_ret=None), 'gamma 1.01': dict(gamma=1.01), 'gamma -0.1': dict(gamma=-0.1),
         'gamma nan': dict(gamma=nan), 'lam inf': dict(lam=inf), 'lam -1': dict(lam=-1.0), 'cost_gamma 2': dict(cost_gamma=2.0),
         'cost_lam nan': dict(cost_lam=nan), 'd_reward + 4': dict(d_reward=b['reward'] + 4), 'd_value + 2': dict(d_value=b['value'] + 2),
         'd_cvalue + 1': dict(d_cvalue=b['cvalue'] + 1), 'd_slot + 2': dict(d_slot=b['slot'] + 2), 'd_final_value + 1': dict(d_final_value=b['fv'] + 1),
         'd_final_cvalue + 3': dict(d_final_cvalue=b['fcv'] + 3), 'd_adv + 2': dict(d_adv=b['adv'] + 2), 'd_ret + 1': dict(d_ret=b['ret'] + 1),
         'd_cadv + 2': dict(d_cadv=b['cadv'] + 2), 'd_cret + 2': dict(d_cret=b['cret'] + 2),
         'cost outputs without d_cvalue': dict(d_cvalue=None), 'd_cvalue without d_cadv': dict(d_cadv=None),
         'd_cvalue without d_cret': dict(d_cret=None), 'slots with capacity 0': dict(capacity=0), 'slots with capacity -2': dict(capacity=-2)}
  for what, change in bad.items():
    g.clear_outputs()
    d = g.desc(nat, 0.99, 0.95, 0.99, 0.95, 8, **change)
    rc = ctx.lib.sag_gae_device(ctx.h, C.byref(d))
    ctx.wait()
    assert rc == ERR_ARG, f'{what}: {rc}'
    for k, o in g.outputs().items():
      assert (o == OUT_FILL).all(), f'{what}: {k} was written'
  g.clear_outputs()
  assert ctx.lib.sag_gae_device(ctx.h, None) == ERR_ARG
  assert ctx.lib.sag_gae_device(ctx.h, C.byref(g.desc(nat, 0.99, 0.95, 0.99, 0.95, 8))) == 0   # the context is usable after the refusals
  ctx.wait()
  assert (g.outputs()['adv'][:, :N] != OUT_FILL).all()
  g.free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. sag.RolloutBuffer against the loop written by hand
# ---------------------------------------------------------------------------------------------------------------------
def _hand_rollout(B, acts):
  """env.step(sync=True) with final_observation=True, every return downloaded."""
  out = {k: [] for k in ('obs', 'reward', 'done', 'cost', 'terminated', 'goal_met', 'episode', 'final')}
  for a in acts:
    obs, rew, done, info = B.step(a)
    for k, v in (('obs', obs), ('reward', rew), ('done', done), ('cost', info['cost']), ('terminated', info['terminated']),
                 ('goal_met', info['goal_met']), ('episode', info['episode']), ('final', info['final_observation'])):
      out[k].append(_np(v).copy())
  return {k: np.stack(v) for k, v in out.items()}


def _compare(buf, hand, what):
  got = {k: getattr(buf, k).numpy() for k in ('obs', 'reward', 'done', 'cost', 'terminated', 'goal_met', 'episode', 'final_slot')}
  T = buf.T
  if hand['reward'].ndim == 3:   # (a task with a second reward column: the buffer's view is column 0)
    hand = dict(hand, reward=hand['reward'][..., 0])
  np.testing.assert_array_equal(got['obs'][1:].view(np.uint32), hand['obs'].view(np.uint32), err_msg=f'{what}: obs[t + 1]')
  np.testing.assert_array_equal(got['reward'].view(np.uint32), hand['reward'].view(np.uint32), err_msg=f'{what}: reward')
  for k in ('done', 'cost', 'terminated', 'goal_met'):
    np.testing.assert_array_equal(got[k], hand[k], err_msg=f'{what}: {k}')
  e = got['done'] != 0
  np.testing.assert_array_equal(got['episode'][e].view(np.uint32), hand['episode'][e].view(np.uint32), err_msg=f'{what}: episode rows')
  rows, count = buf.final_observations()
  assert count == e.sum() and buf.final_dropped() == 0, (what, count, e.sum())
  rows = rows.numpy()
  assert rows.shape == (count, buf.obs_dim)
  slot = got['final_slot']
  assert (slot[~e] == -1).all() and sorted(slot[e]) == list(range(count)), what
  for t in range(T):
    for i in np.flatnonzero(e[t]):
      np.testing.assert_array_equal(rows[slot[t, i]].view(np.uint32), hand['final'][t, i].view(np.uint32),
                                    err_msg=f'{what}: final row of env {i} at step {t}')
  return got


@pytest.mark.gpu
@pytest.mark.parametrize('robot,task', [('point', 'go_to_goal'), ('car', 'push_box'), ('doggo', 'go_to_goal')])
def test_rollout_buffer_equals_the_loop_written_by_hand(nat, robot, task):
  """Two envs of 130 from one seed, time_limit 7 and auto_reset; B also final_observation.  Three warm-up steps and the same
  masked reset of a random third de-phase the episodes; then 20 steps with the same host-drawn actions, A through the
  buffer, B through env.step(sync=True).  Everything the buffer stored equals what B returned, bit for bit; a second rollout
  continues from obs[T]; advantages() equals gae_ref32 on the downloaded arrays."""
  import safe_adaptation_gym_amd as sag
  T, limit = 20, 7
  kw = dict(n_envs=N, seed=61, device_buffers=True, time_limit=limit, auto_reset=True)
  A, B = _make_env(robot, task, **kw), _make_env(robot, task, final_observation=True, **kw)
  np.testing.assert_array_equal(_np(A.reset()), _np(B.reset()))
  rng = np.random.RandomState(11)
  nu = A.robot.nu
  for _ in range(3):
    act = rng.uniform(-1, 1, (N, nu)).astype(np.float32)
    A.step(act)
    B.step(act)
  m = rng.rand(N) < 1 / 3
  assert 0 < m[:64].sum() < 64 and 0 < m[64:128].sum() < 64
  start = _np(A.reset(mask=m))
  np.testing.assert_array_equal(start, _np(B.reset(mask=m)))
  buf = sag.RolloutBuffer(A, steps=T)
  assert buf.final_capacity == N * (T // limit + 1)
  with pytest.raises(ValueError):
    buf.step(0)   # before begin()
  seen_trunc = seen_partial = False
  last_obs = None
  for r in range(2):
    acts = rng.uniform(-1, 1, (T, N, nu)).astype(np.float32)
    buf.begin()
    with pytest.raises(ValueError):
      buf.step(1)   # out of order
    for t in range(T):
      buf.set_actions(t, acts[t])
      buf.step(t)
    with pytest.raises(ValueError):
      buf.step(T)
    buf.wait()
    hand = _hand_rollout(B, acts)
    got = _compare(buf, hand, f'{robot}, rollout {r}')
    np.testing.assert_array_equal(got['obs'][0].view(np.uint32), (start if r == 0 else last_obs).view(np.uint32),
                                  err_msg=f'rollout {r}: obs[0]')
    np.testing.assert_array_equal(buf.actions.numpy(), acts)
    last_obs = got['obs'][T]
    e = got['done'] != 0
    seen_trunc |= bool((got['done'] == 2).any())
    seen_partial |= bool(((e.sum(1) > 0) & (e.sum(1) < N)).any())
  assert seen_trunc and seen_partial, 'the rollouts show nothing: no truncation, or no step with a partial mask'
  # advantages of the last rollout, host values
  rows, count = buf.final_observations()
  value, cvalue = rng.normal(0, 3, (T + 1, N)).astype(np.float32), rng.normal(1, 1, (T + 1, N)).astype(np.float32)
  fv, fcv = rng.normal(0, 3, count).astype(np.float32), rng.normal(1, 1, count).astype(np.float32)
  out = buf.advantages(value, cvalue, fv, fcv, gamma=0.99, lam=0.95, cost_gamma=0.995, cost_lam=0.9)
  buf.wait()
  cap = buf.final_capacity
  full = lambda x: np.concatenate([x, np.zeros(cap - count, np.float32)])   # noqa: E731
  want = R.gae_ref32(got['reward'], got['cost'], got['done'], value, 0.99, 0.95, got['final_slot'], full(fv), cap) + \
      R.gae_ref32(None, got['cost'], got['done'], cvalue, 0.995, 0.9, got['final_slot'], full(fcv), cap, is_cost=True)
  for k, w in zip(('adv', 'ret', 'cadv', 'cret'), want):
    assert out[k].shape == (T, N)
    np.testing.assert_array_equal(out[k].numpy().view(np.uint32), w.view(np.uint32), err_msg=k)
  # the reward channel alone, no final values: truncations bootstrap from zero; the device views as inputs
  buf.value.ctx.dev_upload(nat.C.c_void_p(buf.value.ptr), np.pad(value, ((0, 0), (0, buf.P - N))))
  out = buf.advantages(buf.value, gamma=1.0, lam=1.0)
  assert set(out) == {'adv', 'ret'}
  want = R.gae_ref32(got['reward'], got['cost'], got['done'], value, 1.0, 1.0)
  np.testing.assert_array_equal(out['adv'].numpy().view(np.uint32), want[0].view(np.uint32))
  np.testing.assert_array_equal(out['ret'].numpy().view(np.uint32), want[1].view(np.uint32))
  # the env still steps on its own, and a rollout may follow it
  own = _np(A.step(acts[0])[0]).copy()
  np.testing.assert_array_equal(own, _np(B.step(acts[0])[0]))
  buf.begin(from_env=True)
  buf.wait()
  np.testing.assert_array_equal(buf.obs[0].numpy(), own)
  buf.close()
  assert A.reset_counts()[1] == 0 and B.reset_counts()[1] == 0
  A.close(); B.close()


@pytest.mark.gpu
def test_rollout_buffer_counts_final_rows_that_do_not_fit(nat):
  """final_capacity=5 under time_limit 2: every env is truncated at once, five rows are kept and the rest counted."""
  import safe_adaptation_gym_amd as sag
  n = 70
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=3, device_buffers=True, time_limit=2, auto_reset=True)
  env.reset()
  buf = sag.RolloutBuffer(env, steps=4, final_capacity=5)
  buf.collect(lambda obs, act: act.ctx.dev_upload(nat.C.c_void_p(act.ptr), np.zeros(act.shape, np.float32)))
  rows, count = buf.final_observations()
  done, slot = buf.done.numpy(), buf.final_slot.numpy()
  total = int((done != 0).sum())
  assert total >= 2 * n and count == 5 and rows.shape == (5, env.robot.obs_dim) and buf.final_dropped() == total - 5
  assert sorted(slot[slot >= 0]) == list(range(5)) and (slot[done == 0] == -1).all()
  out = buf.advantages(np.zeros((5, n), np.float32), final_value=np.ones(5, np.float32), gamma=1.0, lam=0.0)
  adv, rew = out['adv'].numpy(), buf.reward.numpy()
  np.testing.assert_array_equal(adv, (rew + (slot >= 0)).astype(np.float32))   # a kept truncation bootstraps from 1, a dropped one from 0
  buf.close(); env.close()


@pytest.mark.gpu
def test_rollout_buffer_refuses_what_it_cannot_serve(nat):
  """Every ValueError of the constructor, each on an env that still steps afterwards."""
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import benchmark
  task = benchmark.TASKS['go_to_goal']
  dev = dict(device_buffers=True, device_reset=True)

  def steps(env):
    env.reset()
    env.step(np.zeros((env.n_envs, env.robot.nu), np.float32))
    env.close()

  with pytest.raises(ValueError, match='BatchedSafeAdaptationGym'):
    sag.RolloutBuffer(object(), steps=4)
  cases = {'device_buffers': dict(device_reset=True), 'auto_reset': dict(time_limit=5, **dev), 'parity_rng': dict(parity_rng=True),
           'sharded': dict(auto_reset=True, devices=[0, 0], **dev)}
  for match, kw in cases.items():
    env = sag.make('point', None, n_envs=8, **kw)
    env.set_task(task)
    with pytest.raises(ValueError, match=match):
      sag.RolloutBuffer(env, steps=4)
    steps(env)
  env = sag.make('point', None, n_envs=8, auto_reset=True, **dev)
  with pytest.raises(ValueError, match='task'):
    sag.RolloutBuffer(env, steps=4)
  env.set_task(task)
  for kw in (dict(steps=0), dict(steps=4, final_capacity=0)):
    with pytest.raises(ValueError):
      sag.RolloutBuffer(env, **kw)
  steps(env)
  env = sag.make('point', None, n_envs=8, rgb_observation=True, **dev)
  env.episode_loop(auto_reset=True)
  env.set_task(task)
  with pytest.raises(ValueError, match='image'):
    sag.RolloutBuffer(env, steps=4)
  steps(env)

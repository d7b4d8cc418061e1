"""The learner's reductions and elementwise kernels on the device (csrc/sag_learner.hpp: sag_moments_device,
sag_advantage_mix_device, sag_lagrange_device, sag_grad_clip_device) against the NumPy restatement of tests/learner_ref.py,
which test_learner_ref.py pins - never against the kernels' own arithmetic.

The two reductions are defined to a tolerance.  Per case the error of the float32 restatement (every term added one after the
other, against the float64 one) is computed, and the device is granted 8 times the largest of its measures: it adds the same
fp32 terms in another order.  An indexing fault costs a whole element, >= 1 / n of the result.  Where a tolerance could hide one
(large n) the exact cases take over: inputs that are integers in -2 ... 2 make every fp32 partial sum exact for any grid, so
count and sum must be the integers; a constant with a two-bit mantissa must give var == 0.  The mix and the multiplier are
elementwise and compared bit for bit.  Shapes: a block's unit is 4096 elements, the default grid cap 256 blocks, the hard cap
1024 - so 1, 33 x 3 pitched, sizes that end inside a unit and inside a quad, 256 x 4096 + 1 (a block takes a second chunk) and
1024 x 4096 + 1 under max_blocks = 4096.  The cases below the default cap also run on the host build of the device sources
(test_learner_kernels_hostemu.py)."""
import ctypes as C

import numpy as np
import pytest

import learner_ref as R
from test_device_reset import KEY

F32, F64 = np.float32, np.float64
ERR_ARG = -1
GUARD = 8
SENTINEL = 7.0
FACTOR = 8.0
UNIT = 4096
EPS = 1e-8


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(nat):
  c = nat.Context('point', 8, seed=KEY)
  yield c
  c.close()


class _Buf:
  """A device buffer that holds exactly `host` (any dtype), freed by free()."""

  def __init__(self, c, host):
    self.c, self.host = c, np.ascontiguousarray(host)
    self.p = c.dev_alloc(max(self.host.nbytes, 4))
    c.dev_upload(self.p, self.host)

  def at(self, byte_offset=0):
    return self.p.value + byte_offset

  def get(self):
    return self.c.dev_download(self.p, self.host.shape, self.host.dtype)

  def free(self):
    self.c.dev_free(self.p)


def _out(c, words):
  return _Buf(c, np.full(words + GUARD, SENTINEL, F32))


def _guarded(buf, words):
  w = buf.get()
  assert (w[words:] == F32(SENTINEL)).all(), 'a write behind the output'
  return w[:words]


def _layout(values, n_rows, n_planes, pitch, stride=1, lead=0):
  """The logical values [n_planes * n_rows] laid out at (p * pitch + r) * stride behind `lead` floats, NaN everywhere else; the
  array ends with the last counted row's own column (a kernel that reads a pad row or another column past it leaves the
  allocation)."""
  n = lead + ((n_planes - 1) * pitch + n_rows - 1) * stride + 1
  x = np.full(n, np.nan, F32)
  idx = (np.arange(n_planes)[:, None] * pitch + np.arange(n_rows)[None, :]).reshape(-1)
  x[lead + idx * stride] = values
  return x


def _moments(c, x, n_rows, n_planes, pitch, stride=1, lead=0, mask=None, max_blocks=0, eps=EPS, wait=True):
  bx, bo = _Buf(c, x), _out(c, 4)
  bm = _Buf(c, mask) if mask is not None else None
  c.moments(n_rows, n_planes, pitch, bx.at(4 * lead), bo.p, d_mask=bm.p if bm else None, stride=stride, eps=eps, max_blocks=max_blocks)
  if not wait:
    return bx, bo, bm
  c.wait()
  got = _guarded(bo, 4)
  for b in (bx, bo, bm):
    if b:
      b.free()
  return got


def _check_moments(got, values, what):
  ref = R.moments64(values, EPS)
  own = R.moments_measure(R.moments32(values, EPS), ref)
  tol = FACTOR * max(own.values())
  m = R.moments_measure(got, ref)
  print(f'{what}: tolerance {tol:.3e}, restatement ' + ' '.join(f'{k} {v:.2e}' for k, v in own.items()) + ', device ' +
        ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
  assert got[0] == ref[0], f'{what}: count {got[0]} for {ref[0]}'
  bad = {k: v for k, v in m.items() if not v <= tol}
  assert not bad, f'{what}: {bad} beyond {tol:.3e}'


# (name, n_rows, n_planes, pitch, lead floats, max_blocks)
MOMENT_SHAPES = [
    ('one element', 1, 1, 1, 0, 0),
    ('33 x 3 pitched', 33, 3, 38, 0, 0),
    ('ends inside a unit, planes end inside a quad', 1667, 3, 1668, 0, 0),
    ('contiguous from an odd word', 5001, 2, 5001, 1, 0),
    ('256 units and one element: a second chunk', 256 * UNIT + 1, 1, 256 * UNIT + 1, 0, 0),
    ('1024 units and one element under max_blocks 4096', 1024 * UNIT + 1, 1, 1024 * UNIT + 1, 0, 4096),
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(MOMENT_SHAPES)), ids=[s[0] for s in MOMENT_SHAPES])
def test_moments_against_the_reference(ctx, case):
  """mean, var and rstd within 8 x the float32 restatement's own error of the float64 one, the count exact, NaN in every pad
  row, and nothing written behind the four words."""
  name, n_rows, n_planes, pitch, lead, mb = MOMENT_SHAPES[case]
  values = np.random.RandomState(100 + case).normal(0.3, 2.0, n_rows * n_planes).astype(F32)
  got = _moments(ctx, _layout(values, n_rows, n_planes, pitch, 1, lead), n_rows, n_planes, pitch, 1, lead, max_blocks=mb)
  _check_moments(got, values, name)


@pytest.mark.gpu
def test_moments_strided_masked_and_poisoned(ctx):
  """The cost column of [3][40][4] episode rows (d_x = episode + 1, stride 4) under a `done` mask: NaN in the three other
  columns, in every pad row and under every zero mask byte; non-zero mask bytes of any value count; the mask's pad bytes are
  set and must not count."""
  rng = np.random.RandomState(7)
  n_rows, n_planes, pitch = 33, 3, 40
  values = rng.normal(20.0, 6.0, n_rows * n_planes).astype(F32)
  keep = rng.uniform(size=n_rows * n_planes) < 0.3
  mask = np.full((n_planes, pitch), 1, np.uint8)
  mask[:, :n_rows] = (keep * rng.randint(1, 256, keep.size)).reshape(n_planes, n_rows)
  x = _layout(np.where(keep, values, np.nan), n_rows, n_planes, pitch, 4, 1)
  got = _moments(ctx, x, n_rows, n_planes, pitch, 4, 1, mask=mask)
  assert keep.sum() > 8
  _check_moments(got, values[keep], 'strided, masked')
  # the same mask over a plain array, from a mask address that is not a multiple of 4
  x1 = _layout(np.where(keep, values, np.nan), n_rows, n_planes, pitch)
  bx, bo, bm = _Buf(ctx, x1), _out(ctx, 4), _Buf(ctx, np.concatenate([np.zeros(1, np.uint8), mask.reshape(-1)]))
  ctx.moments(n_rows, n_planes, pitch, bx.p, bo.p, d_mask=bm.at(1), eps=EPS)
  ctx.wait()
  _check_moments(_guarded(bo, 4), values[keep], 'masked, odd mask address')
  for b in (bx, bo, bm):
    b.free()


@pytest.mark.gpu
def test_moments_empty_and_single_mask(ctx):
  n_rows, n_planes, pitch = 33, 3, 36
  x = _layout(np.full(n_rows * n_planes, np.nan, F32), n_rows, n_planes, pitch)
  mask = np.zeros((n_planes, pitch), np.uint8)
  got = _moments(ctx, x, n_rows, n_planes, pitch, mask=mask)
  assert got.tobytes() == np.zeros(4, F32).tobytes(), got
  mask[2, 31] = 200
  x[2 * pitch + 31] = F32(-3.25)
  got = _moments(ctx, x, n_rows, n_planes, pitch, mask=mask)
  np.testing.assert_array_equal(got, R.moments32(np.array([-3.25], F32), EPS))
  assert got[0] == 1 and got[1] == F32(-3.25) and got[2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize('n_rows,n_planes,pitch,mb', [(33, 3, 38, 0), (3 * UNIT + 5, 2, 3 * UNIT + 8, 0), (257 * UNIT + 3, 1, 257 * UNIT + 3, 0),
                                                      (257 * UNIT + 3, 1, 257 * UNIT + 3, 300)])
def test_moments_exact_on_small_integers_and_constants(ctx, n_rows, n_planes, pitch, mb):
  """Integers in -2 ... 2: every fp32 partial sum is an integer below 2^24 and so exact whatever the grid - count must be n,
  mean the correctly rounded sum / n (so round(mean * n) is the sum: an element dropped or taken twice moves it by >= 1 unless
  it is a 0, and the count catches those).  A constant 1.5 (sums exact likewise): mean 1.5 and var 0 exactly."""
  n = n_rows * n_planes
  k = np.random.RandomState(n_rows).randint(-2, 3, n)
  got = _moments(ctx, _layout(k.astype(F32), n_rows, n_planes, pitch), n_rows, n_planes, pitch, max_blocks=mb)
  total = int(k.sum())
  assert got[0] == n
  assert got[1] == F32(F64(total) / F64(F32(n))), (got[1], total)
  assert round(float(F64(got[1]) * n)) == total
  got = _moments(ctx, _layout(np.full(n, 1.5, F32), n_rows, n_planes, pitch), n_rows, n_planes, pitch, max_blocks=mb)
  assert got[0] == n and got[1] == F32(1.5) and got[2] == 0 and got[3] == F32(F32(1) / F32(EPS))


@pytest.mark.gpu
def test_moments_repeat_and_workspace_growth(nat):
  """The same call twice: the same bits.  On a fresh context (no workspace yet) a one-block call is enqueued and, without a
  wait, a 256-block call that has to replace the workspace: the first call's result is that of a later repeat, bit for bit."""
  c = nat.Context('point', 8, seed=KEY)
  try:
    rng = np.random.RandomState(11)
    small = rng.normal(size=33 * 3).astype(F32)
    big = rng.normal(size=256 * UNIT + 1).astype(F32)
    xs, xb = _layout(small, 33, 3, 38), big
    first = _moments(c, xs, 33, 3, 38, wait=False)
    second = _moments(c, xb, big.size, 1, big.size, wait=False)
    c.wait()
    a, b = _guarded(first[1], 4), _guarded(second[1], 4)
    again_small = _moments(c, xs, 33, 3, 38)
    again_big = _moments(c, xb, big.size, 1, big.size)
    assert a.tobytes() == again_small.tobytes() and b.tobytes() == again_big.tobytes()
    _check_moments(a, small, 'the call queued ahead of the growth')
    _check_moments(b, big, 'the call that grew the workspace')
    for t in first + second:
      if t:
        t.free()
  finally:
    c.close()


# ---- the mix ----
def _mix_case(c, n_rows, n_planes, pitch, adv_mode, cadv_mode, cost, lam_on_device, lead=0, seed=0):
  rng = np.random.RandomState(seed)
  n = n_rows * n_planes
  adv, cadv = rng.normal(0.5, 3.0, n).astype(F32), rng.normal(4.0, 9.0, n).astype(F32)
  ma, mc = R.moments32(adv, EPS), R.moments32(cadv, EPS)
  lam = F32(0.731)
  ba, bc = _Buf(c, _layout(adv, n_rows, n_planes, pitch, 1, lead)), _Buf(c, _layout(cadv, n_rows, n_planes, pitch, 1, lead))
  bma, bmc, bl = _Buf(c, ma), _Buf(c, mc), _Buf(c, np.array([lam, np.nan, np.nan, np.nan], F32))
  words = lead + n_planes * pitch
  bo = _out(c, words)
  c.advantage_mix(n_rows, n_planes, pitch, ba.at(4 * lead), bo.at(4 * lead), d_cadv=bc.at(4 * lead) if cost else None, adv_mode=adv_mode,
                  cadv_mode=cadv_mode, d_adv_mom=bma.p if adv_mode else None, d_cadv_mom=bmc.p if cost and cadv_mode else None,
                  d_lambda=bl.p if lam_on_device else None, cost_weight=123.0 if lam_on_device else lam)
  c.wait()
  got = _guarded(bo, words)[lead:].reshape(n_planes, pitch)
  want = R.mix32(adv, cadv if cost else None, adv_mode, cadv_mode, ma, mc, lam).reshape(n_planes, n_rows)
  assert got[:, :n_rows].tobytes() == want.tobytes(), (adv_mode, cadv_mode, cost, np.abs(got[:, :n_rows] - want).max())
  assert (got[:, n_rows:] == F32(SENTINEL)).all(), 'a pad row of the output was written'
  assert (_guarded(bo, words)[:lead] == F32(SENTINEL)).all()
  for b in (ba, bc, bma, bmc, bl, bo):
    b.free()


@pytest.mark.gpu
@pytest.mark.parametrize('adv_mode', [0, 1, 2])
@pytest.mark.parametrize('cadv_mode', [0, 1, 2])
def test_mix_equals_the_restatement_bit_for_bit(ctx, adv_mode, cadv_mode):
  """Every mode pair on 33 x 3 rows at a pitch of 38 (NaN pad rows in both inputs, the output's pad rows keep their sentinel),
  lambda from the desc and from the device; on 64 x 2 rows at a pitch of 64 (every quad one 16-byte access); and from an odd
  word (no quad aligned)."""
  for lam_on_device in (False, True):
    _mix_case(ctx, 33, 3, 38, adv_mode, cadv_mode, True, lam_on_device, seed=3 * adv_mode + cadv_mode)
  _mix_case(ctx, 64, 2, 64, adv_mode, cadv_mode, True, True, seed=20)
  _mix_case(ctx, 67, 2, 68, adv_mode, cadv_mode, True, False, lead=1, seed=21)


@pytest.mark.gpu
@pytest.mark.parametrize('adv_mode', [0, 1, 2])
def test_mix_without_a_cost_channel(ctx, adv_mode):
  _mix_case(ctx, 33, 3, 38, adv_mode, 2, False, False, seed=30)
  _mix_case(ctx, 64, 2, 64, adv_mode, 0, False, True, seed=31)


# ---- the multiplier ----
@pytest.mark.gpu
def test_lagrange_sequence_equals_the_restatement(ctx):
  """Five updates from lambda 0.1 with lr 0.05, budget 25, lambda_max 0.5: a rise, a fall, no episodes (only word 2 moves), the
  clamp at 0 and the clamp at lambda_max - after each the four words equal lagrange32 bit for bit."""
  lr, budget, cap = 0.05, 25.0, 0.5
  moms = [[12, 28.37, 1.0, 1.0], [7, 23.9, 2.0, 0.5], [0, 0, 0, 0], [3, 2.125, 0.0, 1e8], [40, 61.03, 9.0, 0.3]]
  state = np.array([0.1, 0, 0, 0], F32)
  bs = _Buf(ctx, np.concatenate([state, np.full(GUARD, SENTINEL, F32)]))
  seen = []
  for mom in moms:
    bm = _Buf(ctx, np.array(mom, F32))
    ctx.lagrange(bm.p, bs.p, lr, budget, cap)
    ctx.wait()
    before, state = state, R.lagrange32(state, np.array(mom, F32), lr, budget, cap)
    got = bs.get()
    assert got[:4].tobytes() == state.tobytes(), (got[:4], state)
    assert (got[4:] == F32(SENTINEL)).all()
    seen.append((float(before[0]), float(state[0])))
    bm.free()
  bs.free()
  assert seen[0][1] > seen[0][0] and seen[1][1] < seen[1][0] and seen[2][1] == seen[2][0] and seen[3][1] == 0.0 and seen[4][1] == 0.5
  assert state[3] == 4 and state[2] == 40


# ---- the clip ----
POINT32_PARAMS = 60 * 32 + 32 + 32 * 32 + 32 + 32 * 4 + 4 + 2


def _clip(c, g, max_norm, max_blocks=0):
  n = g.size
  behind = np.arange(1, 9, dtype=F32)   # the 8 statistics behind a gradient
  bg = _Buf(c, np.concatenate([g, behind, np.full(GUARD, SENTINEL, F32)]))
  bo = _out(c, 2)
  c.grad_clip(n, bg.p, bo.p, max_norm, max_blocks=max_blocks)
  c.wait()
  w = bg.get()
  assert w[n:n + 8].tobytes() == behind.tobytes() and (w[n + 8:] == F32(SENTINEL)).all(), 'a write behind the gradient'
  out = _guarded(bo, 2)
  bg.free(); bo.free()
  return out[0], out[1], w[:n]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 33, POINT32_PARAMS, 256 * UNIT + 1])
def test_clip_norm_factor_and_scaling(ctx, n):
  """The norm within 8 x the float32 restatement's own error; under a max_norm above it the factor is 1 and every bit of the
  gradient and of the 8 words behind it stays; under half the norm every element is fl(g * factor) for the factor the device
  wrote, which is fl(max_norm / fl(norm + 1e-6)) of the norm it wrote."""
  g = np.random.RandomState(200 + n % 97).normal(0.0, 0.02, n).astype(F32)
  n64, _ = R.clip64(g, 1.0)
  own = abs(F64(R.clip32(g, 1.0)[0]) - n64) / n64
  norm, factor, out = _clip(ctx, g, 2.0 * n64)
  err = abs(F64(norm) - n64) / n64
  print(f'clip n = {n}: tolerance {FACTOR * own:.3e}, restatement {own:.2e}, device {err:.2e}')
  assert err <= FACTOR * own
  assert factor == 1 and out.tobytes() == g.tobytes()
  norm2, factor, out = _clip(ctx, g, 0.5 * n64)
  assert norm2 == norm
  assert factor == F32(F32(0.5 * n64) / F32(norm + F32(1e-6))) and factor < 1
  assert out.tobytes() == R.scale32(g, factor).tobytes()


@pytest.mark.gpu
def test_clip_of_a_zero_gradient(ctx):
  norm, factor, out = _clip(ctx, np.zeros(POINT32_PARAMS, F32), 0.5)
  assert norm == 0 and factor == 1 and not out.any()


# ---- refusals ----
@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(nat, ctx):
  """Every SAG_ERR_ARG condition of the four functions: the return code, and every output still its sentinel."""
  c = ctx
  x = _Buf(c, np.ones(64, F32))
  m = _Buf(c, np.ones(64, np.uint8))
  o = _Buf(c, np.full(64, SENTINEL, F32))
  inf, nan = float('inf'), float('nan')

  def refused(fn, desc):
    rc = fn(c.h, C.byref(desc) if desc is not None else None)
    c.wait()
    assert rc == ERR_ARG, (fn.__name__, rc)
    assert (o.get() == F32(SENTINEL)).all() and (x.get() == 1).all()

  L = c.lib
  def mom(**kw):
    d = dict(n_rows=4, n_planes=2, pitch=8, stride=1, max_blocks=0, reserved=0, eps=1e-8, reserved_f=0.0, d_x=x.at(), d_mask=m.at(), d_out=o.at())
    d.update(kw)
    return nat.MomentsDesc(**d)
  refused(L.sag_moments_device, None)
  for kw in (dict(d_x=None), dict(d_out=None), dict(d_x=x.at(2)), dict(d_out=o.at(1)), dict(pitch=3), dict(n_rows=0), dict(n_planes=0),
             dict(stride=0), dict(n_rows=1 << 16, pitch=1 << 16, n_planes=1 << 15), dict(max_blocks=-1), dict(eps=nan), dict(eps=inf),
             dict(eps=-1.0)):
    refused(L.sag_moments_device, mom(**kw))

  def mix(**kw):
    d = dict(n_rows=4, n_planes=2, pitch=8, reserved=0, adv_mode=2, cadv_mode=1, cost_weight=0.5, reserved_f=0.0, d_adv=x.at(), d_cadv=x.at(64),
             d_adv_mom=x.at(128), d_cadv_mom=x.at(144), d_lambda=None, d_out=o.at())
    d.update(kw)
    return nat.AdvantageMixDesc(**d)
  refused(L.sag_advantage_mix_device, None)
  for kw in (dict(d_adv=None), dict(d_out=None), dict(d_adv_mom=None), dict(d_cadv_mom=None), dict(d_adv=x.at(2)), dict(d_cadv=x.at(66)),
             dict(d_adv_mom=x.at(130)), dict(d_cadv_mom=x.at(146)), dict(d_lambda=x.at(3)), dict(d_out=o.at(2)), dict(pitch=3), dict(n_rows=0),
             dict(n_planes=0), dict(n_rows=1 << 16, pitch=1 << 16, n_planes=1 << 15), dict(adv_mode=3), dict(adv_mode=-1), dict(cadv_mode=3),
             dict(cost_weight=nan), dict(cost_weight=inf)):
    refused(L.sag_advantage_mix_device, mix(**kw))

  def lag(**kw):
    d = dict(lr=0.05, budget=25.0, lambda_max=inf, reserved=0.0, d_mom=x.at(), d_state=o.at())
    d.update(kw)
    return nat.LagrangeDesc(**d)
  refused(L.sag_lagrange_device, None)
  for kw in (dict(d_mom=None), dict(d_state=None), dict(d_mom=x.at(1)), dict(d_state=o.at(2)), dict(lr=nan), dict(lr=inf), dict(lr=-0.1),
             dict(budget=nan), dict(budget=inf), dict(lambda_max=nan), dict(lambda_max=-1.0)):
    refused(L.sag_lagrange_device, lag(**kw))

  def clip(**kw):
    d = dict(n=16, max_blocks=0, max_norm=0.5, reserved=0.0, d_grad=o.at(), d_out=o.at(128))
    d.update(kw)
    return nat.GradClipDesc(**d)
  refused(L.sag_grad_clip_device, None)
  for kw in (dict(d_grad=None), dict(d_out=None), dict(d_grad=o.at(2)), dict(d_out=o.at(130)), dict(n=0), dict(n=-4), dict(max_blocks=-1),
             dict(max_norm=nan), dict(max_norm=inf), dict(max_norm=-1.0), dict(d_out=o.at(0)), dict(d_out=o.at(60)), dict(d_grad=o.at(4), d_out=o.at(0))):
    refused(L.sag_grad_clip_device, clip(**kw))
  # accepted neighbours of the refusals, so that the sentinel check above is not vacuous: the same descs do write
  assert L.sag_grad_clip_device(c.h, C.byref(clip(d_out=o.at(64)))) == 0
  c.wait()
  assert o.get()[16] != F32(SENTINEL)
  for b in (x, m, o):
    b.free()

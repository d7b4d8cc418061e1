"""The shooting planner on the device (csrc/sag_plan.hpp, sag_plan_*_device, planner.ShootingPlanner): sample, score, refit
and the planner that composes them with sag_fork_device.  Every reference is NumPy or the calls that existed before - a twin
context stepped with sag_step_device and an observation buffer, a host-side fork through get_state / set_state -, never the
new code.  The reduced sizes are used on the host build of the device sources."""
import math

import numpy as np
import pytest

import reset_sampler_ref as R
from test_device_reset import KEY
from test_reset_loop import CASES, ENV_ID0, EPISODE0, HOSTEMU, _make, _make_env, _np, _same, _tid, _twin
from test_async_reset import _DevStep
from test_fork import _host_fork

F32 = np.float32
PLAN_WORD = 0x10000000   # counter word 3 of the planner's draws (include/sag.h)
# measured maxima (docstrings of test_refit_equals_numpy / test_sample), asserted with the factor 4 of the issue
SIGMA_MEASURED = 7.401e-8
SAMPLE_MEASURED = 1.564e-7


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


class _Dev:
  """Named device buffers of one context, uploaded from and downloaded to NumPy arrays."""

  def __init__(self, c):
    self.c, self.p, self.meta = c, {}, {}

  def put(self, name, arr):
    arr = np.ascontiguousarray(arr)
    if name not in self.p:
      self.p[name] = self.c.dev_alloc(max(arr.nbytes, 16))
      self.meta[name] = (arr.shape, arr.dtype)
    assert self.meta[name] == (arr.shape, arr.dtype)
    self.c.dev_upload(self.p[name], arr)
    return self.p[name]

  def get(self, name):
    return self.c.dev_download(self.p[name], *self.meta[name])

  def free(self):
    for p in self.p.values():
      self.c.dev_free(p)
    self.p = {}


class _NoContext:
  h = None   # a NULL sag_ctx*


def _with_layout(nat, robot, n):
  c, _, _ = _make(nat, robot, [_tid('go_to_goal')], n)
  assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  return c


# ------------------------------------------------------------------------------------------------------------------
# NumPy restatements
# ------------------------------------------------------------------------------------------------------------------
def _order(ret, cost, budget):
  """The total order of include/sag.h over one group's candidates -> candidate indices, first to last."""
  def key(k):
    r, q = float(ret[k]), float(cost[k])
    if not (math.isfinite(r) and math.isfinite(q)):
      return (2, 0.0, 0.0, k)
    if budget is None or q <= float(budget):
      return (0, -r, 0.0, k)
    return (1, q, -r, k)
  return sorted(range(len(ret)), key=key)


def _refit_ref(plans, score, budget, G, K, E, sigma_min):
  """-> best [G], mean [H, G, nu] (sequential fp32 sum in ascending k, times 1 / E), sigma in float64, the elite sets."""
  H, n, nu = plans.shape
  best, mean, sigma, elites = np.zeros(G, np.int32), np.zeros((H, G, nu), F32), np.zeros((H, G, nu)), []
  inv = F32(1) / F32(E)
  for g in range(G):
    rows = score[g * K:(g + 1) * K]
    order = _order(rows[:, 0], rows[:, 1], None if budget is None else budget[g])
    best[g] = order[0]
    el = sorted(order[:E])
    elites.append(el)
    s = np.zeros((H, nu), F32)
    for k in el:
      s = s + plans[:, g * K + k, :]
    assert s.dtype == F32
    mean[:, g, :] = s * inv
    x = plans[:, g * K + np.array(el), :].astype(np.float64)
    dev = ((x - mean[:, g, None, :].astype(np.float64))**2).sum(axis=1) / E
    sigma[:, g, :] = np.maximum(float(F32(sigma_min)), np.sqrt(dev))
  return best, mean, sigma, elites


def _accumulate_ref(outs, gamma):
  """score [n, 4] from the per-step (reward, cost, done, met) of a rollout: fp32 weight, product and sum."""
  n = len(outs[0][0])
  score, alive, w = np.zeros((n, 4), F32), np.ones(n, bool), F32(1)
  for rew, cost, done, met in outs:
    wr = (w * rew[:, 0].astype(F32)).astype(F32)
    wc = (w * (cost != 0).astype(F32)).astype(F32)
    score[alive, 0] = score[alive, 0] + wr[alive]
    score[alive, 1] = score[alive, 1] + wc[alive]
    score[alive, 2] += F32(1)
    score[alive, 3] += (met != 0).astype(F32)[alive]
    alive &= done == 0
    w = F32(w * F32(gamma))
  return score


def _twin_rollout(dv, plans, gamma):
  """H sag_step_device calls with an observation buffer and downloads, accumulated in NumPy."""
  outs = []
  for t in range(len(plans)):
    o = dv.step(plans[t])
    outs.append((o[1], o[2], o[3], o[4]))
  return _accumulate_ref(outs, gamma)


def _normals_ref(key, id0, n, draw, H, nu):
  """z [H, n, nu]: the Philox words at the counter layout of include/sag.h, the uniforms ((w >> 8) + 0.5) / 2^24 in fp32
  as the action noise forms them (the sum rounds for w >> 8 >= 2^23), then the Box-Muller transform in float64."""
  e = np.arange(H * nu)
  ids = (id0 + np.arange(n))[:, None] + 0 * e[None, :]
  w = R.philox(ids, draw, (e // 4)[None, :] + 0 * ids, PLAN_WORD, key & 0xffffffff, key >> 32)
  hi = (e % 4 >= 2)[None, :]
  wa, wb = np.where(hi, w[2], w[0]), np.where(hi, w[3], w[1])
  u1 = (((wa >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(1 / 16777216.0)).astype(np.float64)
  u2 = (((wb >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(1 / 16777216.0)).astype(np.float64)
  r = np.sqrt(-2.0 * np.log(u1))
  z = np.where((e % 2 == 0)[None, :], r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2))   # [n, H * nu]
  return z.reshape(n, H, nu).transpose(1, 0, 2)


# ------------------------------------------------------------------------------------------------------------------
# 1. refit against NumPy
# ------------------------------------------------------------------------------------------------------------------
def _score_sets(rng, G, K):
  n = G * K
  ret = rng.normal(size=n).astype(F32)
  cost = rng.uniform(0, 5, n).astype(F32)
  steps, goals = rng.randint(1, 9, n).astype(F32), rng.randint(0, 2, n).astype(F32)
  mk = lambda r, q: np.stack([r, q, steps, goals], axis=1).astype(F32)   # noqa: E731
  full = lambda v: np.full(G, v, F32)   # noqa: E731
  per_group = rng.uniform(1, 4, G).astype(F32)
  tie_ret = (np.round(ret * 2) / 2).astype(F32)
  tie_cost = rng.randint(0, 3, n).astype(F32)
  nan_ret = ret.copy()
  nan_ret[np.arange(G) * K + K // 2] = np.nan
  inf_cost = cost.copy()
  inf_cost[np.arange(G) * K + (K - 1) // 3] = np.inf
  return [('all feasible', mk(ret, cost), full(10)), ('none feasible', mk(ret, cost), full(-1)),
          ('mixed', mk(ret, cost), per_group), ('no budget', mk(ret, cost), None),
          ('ties in ret and in cost', mk(tie_ret, tie_cost), full(1)), ('ties, no budget', mk(tie_ret, tie_cost), None),
          ('one NaN ret', mk(nan_ret, cost), per_group), ('one NaN ret and one inf cost, no budget', mk(nan_ret, inf_cost), None)]


@pytest.mark.gpu
@pytest.mark.parametrize('G,K,E,H,nu', [(3, 1, 1, 1, 2), (3, 5, 2, 3, 2), (2, 67, 7, 2, 12), (1, 300, 30, 1, 2)])
def test_refit_equals_numpy(nat, G, K, E, H, nu):
  """sag_plan_refit_device on synthetic plans and scores: `best` and `best_score` equal the NumPy restatement of the
  order, `mean` is bit-equal to the sequential fp32 sum over that restatement's elite set times 1 / E (so the elite sets
  are equal), and sigma is within 4 x the measured maximum of a float64 restatement.
  Measured on the MI355X over every case here: max |sigma - float64 sigma| = 7.401e-8 (G = 2, K = 67, E = 7, nu = 12, one
  NaN ret; sigma is up to 1, so this is about one ulp); the factor 4 covers the host build's libm sqrt and its rounding of
  the deviation sum."""
  n = G * K
  c = _with_layout(nat, 'doggo' if nu == 12 else 'point', n)
  d = _Dev(c)
  rng = np.random.RandomState(100 + K)
  sigma_min = 0.05
  worst = 0.0
  for what, score, budget in _score_sets(rng, G, K):
    plans = rng.uniform(-1, 1, (H, n, nu)).astype(F32)
    if what.startswith('ties'):
      plans[:, 1::2] = plans[:, 0::2][:, :plans[:, 1::2].shape[1]]   # equal plan values too: sigma may reach its floor
    p = {k: d.put(k, v) for k, v in (('plans', plans), ('score', score), ('mean', np.full((H, G, nu), 9, F32)),
                                     ('sigma', np.full((H, G, nu), 9, F32)), ('best', np.full(G, -7, np.int32)),
                                     ('best_score', np.full((G, 4), 9, F32)))}
    pb = None if budget is None else d.put('budget', budget)
    c.plan_refit(K, H, E, p['plans'], p['score'], pb, sigma_min, p['mean'], p['sigma'], p['best'], p['best_score'])
    c.wait()
    best, mean, sigma, elites = _refit_ref(plans, score, budget, G, K, E, sigma_min)
    np.testing.assert_array_equal(d.get('best'), best, err_msg=f'{what}: best')
    np.testing.assert_array_equal(d.get('best_score'), score[np.arange(G) * K + best], err_msg=f'{what}: best_score')
    np.testing.assert_array_equal(d.get('mean'), mean, err_msg=f'{what}: mean (elite sets {elites})')
    got = d.get('sigma')
    assert (got >= F32(sigma_min)).all()
    err = float(np.abs(got.astype(np.float64) - sigma).max())
    worst = max(worst, err)
    print(f'refit G={G} K={K} E={E} {what}: max |sigma - float64| = {err:.3e}')
    assert err <= 4 * SIGMA_MEASURED, f'{what}: sigma off by {err}'
    # without best_score
    c.dev_upload(p['best'], np.full(G, -7, np.int32))
    c.plan_refit(K, H, E, p['plans'], p['score'], pb, sigma_min, p['mean'], p['sigma'], p['best'], None)
    c.wait()
    np.testing.assert_array_equal(d.get('best'), best, err_msg=f'{what}: best without best_score')
  print(f'refit G={G} K={K}: worst sigma error {worst:.3e}')
  d.free(); c.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. score against a twin
# ------------------------------------------------------------------------------------------------------------------
SCORE_N = {'point-mixed': (3 * 67, 3 * 21), 'car-mixed': (2 * 65, 65), 'doggo-mixed': (2 * 35, 35)}


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(SCORE_N))
def test_score_equals_a_stepped_twin(nat, case):
  """A runs sag_plan_score_device on random plans; B, a twin of A under the same key, runs H sag_step_device calls with an
  observation buffer and downloads, and NumPy accumulates with an fp32 weight, product and sum.  H in {1, 5} x gamma in
  {1, 0.9}: the score is bit-equal and so is the state afterwards - leaving the observation out changes nothing."""
  robot, pick, config = CASES[case]
  n = SCORE_N[case][1 if HOSTEMU else 0]
  assert n % 64
  tids, doe = pick(n)
  A, _, _ = _make(nat, robot, tids, n, doe, config=config)
  assert A.reset_device(True, episode0=EPISODE0)[0] == 0
  nu = A.info['nu']
  rng = np.random.RandomState(11)
  for t in range(3):   # (the Doggos land first)
    A.step(rng.uniform(-1, 1, (n, nu)).astype(F32) * (0 if robot == 'doggo' else 1))
  B = _twin(nat, A)
  dv, d = _DevStep(B), _Dev(A)
  for H, gamma in ((1, 1.0), (5, 0.9), (5, 1.0), (1, 0.9)):
    plans = rng.uniform(-1, 1, (H, n, nu)).astype(F32)
    A.plan_score(d.put(f'plans{H}', plans), H, gamma, d.put('score', np.full((n, 4), 7, F32)))
    A.wait()
    got = d.get('score')
    want = _twin_rollout(dv, plans, gamma)
    np.testing.assert_array_equal(got, want, err_msg=f'H={H} gamma={gamma}: score')
    assert (got[:, 2] >= 1).all() and (got[:, 2] <= H).all()
    _same(A.get_state(), B.get_state(), f'H={H} gamma={gamma}: state after the rollout')
  dv.free(); d.free(); A.close(); B.close()


@pytest.mark.gpu
def test_score_counts_a_physics_error_once(nat):
  """A non-finite velocity in two envs (the data path of test_gpu_parity.py::test_physics_error_is_data): their first step
  reports done with reward -10 and cost 0, and their rows count exactly that one step."""
  n, H = 70, 5
  A = _with_layout(nat, 'point', n)
  f, i = A.get_state()
  f[3, 3] = np.nan
  f[66, 0] = np.inf
  A.set_state(f, i)
  B = _twin(nat, A)
  dv, d = _DevStep(B), _Dev(A)
  plans = np.random.RandomState(2).uniform(-1, 1, (H, n, 2)).astype(F32)
  A.plan_score(d.put('plans', plans), H, 0.9, d.put('score', np.zeros((n, 4), F32)))
  A.wait()
  got = d.get('score')
  np.testing.assert_array_equal(got, _twin_rollout(dv, plans, 0.9))
  np.testing.assert_array_equal(got[[3, 66]], np.array([[-10, 0, 1, 0]] * 2, F32))
  ok = np.ones(n, bool); ok[[3, 66]] = False
  assert (got[ok, 2] == H).all()
  _same(A.get_state(), B.get_state(), 'state after the rollout')
  dv.free(); d.free(); A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. sample
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sample(nat):
  """G = 3, K = 67, H = 4 on the Point (nu = 2).  Candidate 0 is clamp(mean); sigma = 0 gives clamp(mean) everywhere;
  mean = +-2 gives +-1; the standardized values of 14 draw words (n = 22 176 >= 20 000) have mean and variance within the
  bounds of tests/test_throughput_rng.py; the same draw gives the same bits, another draw, group or key other values; and
  the values agree with the float64 restatement through reset_sampler_ref.philox.  The tests hold no tolerance for the
  device's action noise against sago_noise (they compare states), so it is measured here: max |plan - float64 plan| =
  1.564e-7 on the MI355X (sigma = 0.5, 14 draws, hardware log2 / sin / cos; 1.269e-7 with the mixed mean and sigma),
  asserted with the factor 4."""
  G, K, H, nu = 3, 67, 4, 2
  n = G * K
  c = _with_layout(nat, 'point', n)
  d = _Dev(c)
  rng = np.random.RandomState(5)
  mean = rng.uniform(-1.3, 1.3, (H, G, nu)).astype(F32)
  sigma = rng.uniform(0.1, 0.6, (H, G, nu)).astype(F32)
  pm, ps, pp = d.put('mean', mean), d.put('sigma', sigma), d.put('plans', np.full((H, n, nu), 9, F32))

  def sample(draw):
    c.plan_sample(K, H, pm, ps, draw, pp)
    c.wait()
    return d.get('plans')

  a = sample(7)
  by_group = a.reshape(H, G, K, nu)
  np.testing.assert_array_equal(by_group[:, :, 0], np.clip(mean, -1, 1), err_msg='candidate 0 is the mean')
  assert (np.abs(a) <= 1).all() and (by_group[:, :, 1:] != np.clip(mean, -1, 1)[:, :, None]).mean() > 0.9
  np.testing.assert_array_equal(sample(7), a, err_msg='the same draw')
  assert (sample(8) != a).reshape(H, G, K, nu)[:, :, 1:].mean() > 0.9, 'another draw'
  # the restatement
  z = _normals_ref(KEY, ENV_ID0, n, 7, H, nu)
  z[:, np.arange(G) * K] = 0
  want = np.clip(np.repeat(mean, K, axis=1).astype(np.float64) + np.repeat(sigma, K, axis=1).astype(np.float64) * z, -1, 1)
  err = float(np.abs(a - want).max())
  print(f'sample: max |plan - float64 plan| = {err:.3e} (mixed mean / sigma)')
  assert err <= 4 * SAMPLE_MEASURED
  c.set_seed(KEY ^ (1 << 40))
  assert (sample(7) != a).reshape(H, G, K, nu)[:, :, 1:].mean() > 0.9, 'another key'
  c.set_seed(KEY)
  # equal mean / sigma in every group: the groups still draw their own values
  c.dev_upload(pm, np.zeros((H, G, nu), F32)); c.dev_upload(ps, np.full((H, G, nu), 0.5, F32))
  worst, zs = 0.0, []
  for draw in range(100, 114):
    b = sample(draw)
    zr = _normals_ref(KEY, ENV_ID0, n, draw, H, nu)
    zr[:, np.arange(G) * K] = 0
    worst = max(worst, float(np.abs(b - np.clip(0.5 * zr, -1, 1)).max()))
    bg = b.reshape(H, G, K, nu)
    assert (bg[:, 0, 1:] != bg[:, 1, 1:]).mean() > 0.9 and (bg[:, 1, 1:] != bg[:, 2, 1:]).mean() > 0.9, 'another group'
  print(f'sample: max |plan - float64 plan| = {worst:.3e} (sigma 0.5, 14 draws)')
  assert worst <= 4 * SAMPLE_MEASURED
  c.dev_upload(ps, np.full((H, G, nu), 0.1, F32))
  for draw in range(100, 114):
    zs.append((sample(draw).reshape(H, G, K, nu)[:, :, 1:].astype(np.float64) / 0.1).ravel())
  x = np.concatenate(zs)
  m = len(x)
  assert m >= 20000 and np.abs(x).max() < 10
  print(f'sample: n = {m}, mean {x.mean():.4f}, var {x.var():.4f}')
  assert abs(x.mean()) < 4 / math.sqrt(m), x.mean()
  assert abs(x.var() - 1) < 4 * math.sqrt(2 / (m - 1)), x.var()
  pairs = x.reshape(14, H, G, K - 1, nu).reshape(-1, 2)   # nu = 2: the two normals of one Box-Muller pair
  assert abs(np.corrcoef(pairs[:, 0], pairs[:, 1])[0, 1]) < 4 / math.sqrt(len(pairs))
  # sigma = 0 and the clamp
  c.dev_upload(pm, mean); c.dev_upload(ps, np.zeros((H, G, nu), F32))
  np.testing.assert_array_equal(sample(3), np.repeat(np.clip(mean, -1, 1), K, axis=1), err_msg='sigma = 0')
  c.dev_upload(ps, np.full((H, G, nu), 0.1, F32))
  for v in (2.0, -2.0):
    c.dev_upload(pm, np.full((H, G, nu), v, F32))
    np.testing.assert_array_equal(sample(3), np.full((H, n, nu), np.sign(v), F32), err_msg=f'mean = {v}')
  d.free(); c.close()


@pytest.mark.gpu
def test_sample_fills_a_short_last_block(nat):
  """H * nu = 6 on the Point and 36 on the Doggo: the last Philox block is used in part (Point) and nu = 12 crosses blocks;
  every element equals the restatement."""
  for robot, G, K, H in (('point', 2, 5, 3), ('doggo', 2, 3, 3)):
    n = G * K
    c = _with_layout(nat, robot, n)
    nu = c.info['nu']
    d = _Dev(c)
    pm, ps = d.put('mean', np.zeros((H, G, nu), F32)), d.put('sigma', np.full((H, G, nu), 0.25, F32))
    pp = d.put('plans', np.full((H + 1, n, nu), 9, F32))
    c.plan_sample(K, H, pm, ps, 2**32 - 1, pp)
    c.wait()
    got = d.get('plans')
    z = _normals_ref(KEY, ENV_ID0, n, 2**32 - 1, H, nu)
    z[:, np.arange(G) * K] = 0
    assert np.abs(got[:H] - np.clip(0.25 * z, -1, 1)).max() <= 4 * SAMPLE_MEASURED
    assert (got[H] == 9).all(), 'a write past the plans'
    d.free(); c.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_of_the_c_calls(nat):
  """Every SAG_ERR_ARG (-1) of the four calls and SAG_ERR_STATE (-4) without a layout, each with the state and every
  buffer untouched."""
  G, K, H, E, nu = 2, 3, 2, 2, 2
  n = G * K
  c = _with_layout(nat, 'point', n)
  c.step(np.zeros((n, nu), F32))
  d = _Dev(c)
  rng = np.random.RandomState(1)
  names = {'plans': rng.rand(H, n, nu), 'mean': rng.rand(H, G, nu), 'sigma': rng.rand(H, G, nu), 'score': rng.rand(n, 4),
           'budget': rng.rand(G), 'best_score': rng.rand(G, 4)}
  p = {k: d.put(k, v.astype(F32)) for k, v in names.items()}
  p['best'] = d.put('best', np.array([-3, -4], np.int32))
  before_state, before = c.get_state(), {k: d.get(k) for k in p}
  off = lambda q, b: nat.C.c_void_p(q.value + b)   # noqa: E731
  nan, inf = float('nan'), float('inf')
  sample = lambda K=K, H=H, m=p['mean'], s=p['sigma'], o=p['plans']: c.plan_sample(K, H, m, s, 1, o)   # noqa: E731
  score = lambda o=p['plans'], H=H, g=0.9, s=p['score']: c.plan_score(o, H, g, s)   # noqa: E731
  refit = lambda K=K, H=H, E=E, o=p['plans'], s=p['score'], b=p['budget'], smin=0.1, m=p['mean'], sg=p['sigma'], be=p['best'], bs=p['best_score']: (   # noqa: E731
      c.plan_refit(K, H, E, o, s, b, smin, m, sg, be, bs))
  shift = lambda G=G, H=H, m=p['mean'], s=p['sigma'], si=0.5: c.plan_shift(G, H, m, s, si)   # noqa: E731
  clear = lambda G=G, H=H, m=p['mean'], s=p['sigma'], si=0.5: c.plan_clear(G, H, None, m, s, si)   # noqa: E731
  bad = [lambda: sample(m=None), lambda: sample(s=None), lambda: sample(o=None), lambda: sample(m=off(p['mean'], 4)),
         lambda: sample(s=off(p['sigma'], 4)), lambda: sample(o=off(p['plans'], 4)), lambda: sample(K=0), lambda: sample(K=-1),
         lambda: sample(K=4), lambda: sample(K=n + 1), lambda: sample(H=0), lambda: sample(H=-2),
         lambda: score(o=None), lambda: score(s=None), lambda: score(o=off(p['plans'], 4)), lambda: score(s=off(p['score'], 4)),
         lambda: score(s=off(p['score'], 8)), lambda: score(H=0), lambda: score(g=0.0), lambda: score(g=-0.5), lambda: score(g=1.5),
         lambda: score(g=nan), lambda: score(g=inf),
         lambda: refit(o=None), lambda: refit(s=None), lambda: refit(m=None), lambda: refit(sg=None), lambda: refit(be=None),
         lambda: refit(o=off(p['plans'], 4)), lambda: refit(s=off(p['score'], 8)), lambda: refit(b=off(p['budget'], 2)),
         lambda: refit(m=off(p['mean'], 4)), lambda: refit(sg=off(p['sigma'], 4)), lambda: refit(be=off(p['best'], 2)),
         lambda: refit(bs=off(p['best_score'], 8)), lambda: refit(K=0), lambda: refit(K=4), lambda: refit(H=0), lambda: refit(E=0),
         lambda: refit(E=K + 1), lambda: refit(E=-1), lambda: refit(smin=-0.1), lambda: refit(smin=nan), lambda: refit(smin=inf),
         lambda: shift(m=None), lambda: shift(s=None), lambda: shift(m=off(p['mean'], 4)), lambda: shift(G=0), lambda: shift(H=0),
         lambda: shift(si=-1.0), lambda: shift(si=nan), lambda: shift(si=inf),
         lambda: clear(m=None), lambda: clear(H=0), lambda: clear(si=nan)]
  for k, call in enumerate(bad):
    with pytest.raises(nat.SagError, match=r'\(-1\)'):
      call()
    c.wait()
    _same(before_state, c.get_state(), f'state after refused call {k}')
    for name in p:
      np.testing.assert_array_equal(d.get(name), before[name], err_msg=f'{name} after refused call {k}')
  with pytest.raises(nat.SagError, match=r'\(-1\)'):
    c.wait_for(_NoContext())
  # without a layout: SAG_ERR_STATE.  The buffers belong to `c`, on the same device; nothing may touch them
  empty = nat.Context('point', n, seed=KEY)
  calls = [lambda: empty.plan_sample(K, H, p['mean'], p['sigma'], 1, p['plans']), lambda: empty.plan_score(p['plans'], H, 0.9, p['score']),
           lambda: empty.plan_refit(K, H, E, p['plans'], p['score'], None, 0.1, p['mean'], p['sigma'], p['best'], None),
           lambda: empty.plan_shift(G, H, p['mean'], p['sigma'], 0.5), lambda: empty.plan_clear(G, H, None, p['mean'], p['sigma'], 0.5)]
  for k, call in enumerate(calls):
    with pytest.raises(nat.SagError, match=r'\(-4\)'):
      call()
    empty.wait()
    for name in p:
      np.testing.assert_array_equal(d.get(name), before[name], err_msg=f'{name} after call {k} without a layout')
  # and the calls are served as given
  sample(); score(); refit(); shift(); clear()
  c.wait()
  assert (d.get('sigma') == 0.5).all() and (d.get('mean') == 0).all()
  empty.close(); d.free(); c.close()


@pytest.mark.gpu
def test_shift_and_clear(nat):
  """sag_plan_shift_device: mean[h] = mean[h + 1], the last row 0, sigma = sigma_init (H = 1 included);
  sag_plan_clear_device with a mask touches the masked groups only."""
  c = _with_layout(nat, 'point', 6)
  d = _Dev(c)
  rng = np.random.RandomState(3)
  for G, H in ((70, 5), (3, 1)):
    mean, sigma = rng.rand(H, G, 2).astype(F32), rng.rand(H, G, 2).astype(F32)
    pm, ps = d.put(f'mean{H}', mean), d.put(f'sigma{H}', sigma)
    c.plan_shift(G, H, pm, ps, 0.3)
    c.wait()
    np.testing.assert_array_equal(d.get(f'mean{H}'), np.concatenate([mean[1:], np.zeros((1, G, 2), F32)]))
    assert (d.get(f'sigma{H}') == F32(0.3)).all()
    c.dev_upload(pm, mean); c.dev_upload(ps, sigma)
    m = (rng.rand(G) < 0.5).astype(np.uint8) * 3
    m[0], m[-1] = 1, 0
    c.plan_clear(G, H, d.put(f'mask{H}', m), pm, ps, 0.4)
    c.wait()
    np.testing.assert_array_equal(d.get(f'mean{H}'), np.where((m != 0)[None, :, None], F32(0), mean))
    np.testing.assert_array_equal(d.get(f'sigma{H}'), np.where((m != 0)[None, :, None], F32(0.4), sigma))
  d.free(); c.close()


@pytest.mark.gpu
def test_planner_refusals(nat):
  """Every ValueError of the constructor."""
  import safe_adaptation_gym_amd as sag
  n = 4
  for kw in ({}, {'device_buffers': True}, {'device_reset': True}, {'parity_rng': True}):
    env = sag.make('point', 'go_to_goal', n_envs=n, seed=5, **kw)
    env.reset()
    with pytest.raises(ValueError):
      sag.ShootingPlanner(env)
    env.close()
  two = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True, devices=[0, 0])
  unset = sag.make('point', None, n_envs=n, seed=5, device_buffers=True, device_reset=True)
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=5, device_buffers=True)
  env.reset()
  before = env.get_state()
  for e, kw in ((two, {}), (unset, {}), (object(), {}), (env, {'candidates': 0}), (env, {'horizon': 0}), (env, {'iterations': 0}),
                (env, {'elites': 0}), (env, {'candidates': 4, 'elites': 5}), (env, {'gamma': 0.0}), (env, {'gamma': 1.5}),
                (env, {'gamma': float('nan')}), (env, {'init_sigma': -1.0}), (env, {'min_sigma': float('inf')}),
                (env, {'cost_budget': np.zeros(n + 1)}), (env, {'cost_budget': float('nan')})):
    with pytest.raises(ValueError):
      sag.ShootingPlanner(e, **kw)
  _same(before, env.get_state(), 'state after refused planners')
  pl = sag.ShootingPlanner(env, candidates=4, horizon=2, iterations=1, elites=2)
  with pytest.raises(ValueError):
    pl.reset(mask=np.zeros(n + 1, bool))
  with pytest.raises(ValueError):
    pl.reset(mask=np.zeros(n, np.float32))
  pl.close()
  for e in (two, unset, env):
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the planner end to end against the composed path
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_planner_equals_the_composed_path(nat):
  """Point / go_to_goal, G = 4, K = 16, H = 4, I = 2, E = 4, budget 0.  After each iteration: the score is bit-equal to the
  twin path of test_score_equals_a_stepped_twin run on the planner's own plans from a host-side fork (_host_fork of
  tests/test_fork.py) of the env's state, `best` equals NumPy's, mean is bit-equal and sigma within the refit test's
  tolerance of the restatement.  The plans are the restatement's draws around the mean the iteration started from.  The
  env's step then reads the action view; the second plan() starts from the shifted mean; and plan() as a whole gives the
  bits of the pieces stepped through here."""
  import safe_adaptation_gym_amd as sag
  G, K, H, I, E, seed = 4, 16, 4, 2, 4, 37
  n = G * K
  kw = dict(candidates=K, horizon=H, iterations=I, elites=E, gamma=0.9, cost_budget=0.0, init_sigma=0.5, min_sigma=0.05)
  envs = [_make_env('point', 'go_to_goal', n_envs=G, seed=seed, device_buffers=True) for _ in range(2)]
  for e in envs:
    e.reset()
    e.step(np.full((G, 2), 0.5, F32))
  env, env2 = envs
  _same(env.get_state(), env2.get_state(), 'two envs made alike')
  pl, pl2 = sag.ShootingPlanner(env, **kw), sag.ShootingPlanner(env2, **kw)
  src = (np.arange(n) // K).astype(np.int32)
  # the twin: a context of n envs under the env's key whose env ids are the planner's
  f, i = env.get_state()
  f, i = np.repeat(f, K, axis=0), np.repeat(i, K, axis=0)
  i[:, R.I_ENV_ID] = np.arange(n)
  T = nat.Context('point', n, seed=env._base_seed)
  T.set_state(f, i)
  dv = _DevStep(T)
  c, b = pl._ctx, pl._bufs
  get = lambda k, shape, dt=F32: c.dev_download(b[k], shape, dt)   # noqa: E731
  budget = np.zeros(G, F32)

  def iterations(first_draw, mean0, sigma0):
    mean, sigma = mean0, sigma0
    for it in range(I):
      pl.iterate()
      c.wait()
      plans, score = get('plans', (H, n, 2)), get('score', (n, 4))
      z = _normals_ref(env._base_seed, 0, n, first_draw + it, H, 2)
      z[:, np.arange(G) * K] = 0
      want = np.clip(np.repeat(mean, K, axis=1).astype(np.float64) + np.repeat(sigma, K, axis=1).astype(np.float64) * z, -1, 1)
      assert np.abs(plans - want).max() <= 4 * SAMPLE_MEASURED, f'iteration {it}: plans'
      _host_fork(T, src, source=env._ctx[0])
      np.testing.assert_array_equal(score, _twin_rollout(dv, plans, 0.9), err_msg=f'iteration {it}: score')
      best, m_ref, s_ref, _ = _refit_ref(plans, score, budget, G, K, E, 0.05)
      k, row = pl.best()
      np.testing.assert_array_equal(k.numpy(), best, err_msg=f'iteration {it}: best')
      np.testing.assert_array_equal(row.numpy(), score[np.arange(G) * K + best], err_msg=f'iteration {it}: best score')
      mean, sigma = get('mean', (H, G, 2)), get('sigma', (H, G, 2))
      np.testing.assert_array_equal(mean, m_ref, err_msg=f'iteration {it}: mean')
      assert np.abs(sigma - s_ref).max() <= 4 * SIGMA_MEASURED, f'iteration {it}: sigma'
    return mean, sigma

  pl.begin()
  mean, sigma = iterations(0, np.zeros((H, G, 2), F32), np.full((H, G, 2), 0.5, F32))
  assert (mean != 0).any()
  act = pl.action()
  assert act.shape == (G, 2) and act.ptr == b['mean'].value
  act2 = pl2.plan()
  np.testing.assert_array_equal(act2.numpy(), mean[0], err_msg='plan() as a whole')
  np.testing.assert_array_equal(act.numpy(), mean[0])
  # the env's step reads the view on its own stream, without a host wait between
  outs, outs2 = env.step(act, sync=False), env2.step(mean[0].copy(), sync=False)
  env.wait(); env2.wait()
  _same(env.get_state(), env2.get_state(), 'the step on the action view')
  _same([_np(outs[0]), _np(outs[1])], [_np(outs2[0]), _np(outs2[1])], 'outputs of the step on the action view')
  # the second plan() starts from the shifted mean
  pl.begin()
  c.wait()
  shifted = np.concatenate([mean[1:], np.zeros((1, G, 2), F32)])
  np.testing.assert_array_equal(get('mean', (H, G, 2)), shifted, err_msg='the shifted mean')
  assert (get('sigma', (H, G, 2)) == F32(0.5)).all()
  mean, sigma = iterations(I, shifted, np.full((H, G, 2), 0.5, F32))
  np.testing.assert_array_equal(pl.action().numpy(), mean[0])
  env2.step(np.zeros((G, 2), F32))   # (env2 is elsewhere now: the planners part ways, pl2 is only closed)
  # reset(mask): the masked envs start over, the others keep their plan
  m = np.array([1, 0, 0, 1], bool)
  pl.reset(mask=m)
  c.wait()
  np.testing.assert_array_equal(get('mean', (H, G, 2)), np.where(m[None, :, None], F32(0), mean))
  np.testing.assert_array_equal(get('sigma', (H, G, 2)), np.where(m[None, :, None], F32(0.5), sigma))
  pl.reset()
  c.wait()
  assert (get('mean', (H, G, 2)) == 0).all() and (get('sigma', (H, G, 2)) == F32(0.5)).all()
  dv.free(); T.close(); pl.close(); pl2.close()
  for e in envs:
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. behaviour
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_planned_envs_approach_their_goals(nat):
  """Point / go_to_goal, G = 8, K = 64, H = 10, I = 2, 30 control steps, no cost budget (host build: G = 2, K = 16, H = 6,
  15 steps).  Three envs from the same start: driven by the planner, by uniform random actions, by zero actions.  The
  distance is taken to the goal each env started with (a goal that is met is drawn anew).  The mean distance of the
  planned envs falls below its initial value and below that of the random twin, and the twin at rest does not reach it
  either."""
  import safe_adaptation_gym_amd as sag
  G, K, H, T = (2, 16, 6, 15) if HOSTEMU else (8, 64, 10, 30)
  envs = [_make_env('point', 'go_to_goal', n_envs=G, seed=91, device_buffers=True) for _ in range(3)]
  for e in envs:
    e.reset()
  planned, random, rest = envs
  f0, _ = planned.get_state()
  goal = f0[:, nat.F_GOAL:nat.F_GOAL + 2].copy()
  dist = lambda e: float(np.linalg.norm(e.get_state()[0][:, nat.F_ROBOT:nat.F_ROBOT + 2] - goal, axis=1).mean())   # noqa: E731
  d0 = dist(planned)
  assert dist(random) == d0 and dist(rest) == d0
  pl = sag.ShootingPlanner(planned, candidates=K, horizon=H, iterations=2, elites=max(2, K // 8), gamma=0.99, cost_budget=None)
  rng = np.random.RandomState(4)
  for t in range(T):
    planned.step(pl.plan(), sync=False)
    random.step(rng.uniform(-1, 1, (G, 2)).astype(F32), sync=False)
    rest.step(np.zeros((G, 2), F32), sync=False)
  for e in envs:
    e.wait()
  d_planned, d_random, d_rest = dist(planned), dist(random), dist(rest)
  print(f'goal distance: start {d0:.4f}, planned {d_planned:.4f}, random {d_random:.4f}, at rest {d_rest:.4f}')
  k, row = pl.best()
  assert k.numpy().shape == (G,) and (row.numpy()[:, 2] >= 1).all()
  assert d_planned < d0 and d_planned < d_random and d_planned < d_rest
  pl.close()
  for e in envs:
    e.close()

"""The device layout of the float state (didx, csrc/sag_device.hpp) and what the step does with it: the free bodies'
positions live in an (x, y) run and a yaw run, the quiet kernel fetches yaw only for an env whose robot is within reach
of something, and the goal group is stored only when the goal moves.

None of that may change a bit of any result.  The round trip catches two record floats on one device float (or one on
none); the rollouts compare the split form (quiet + busy launches, hot records) with the single launch, which loads
every group up front, after every step; the last test pins the one path that must NOT store: a failed env."""
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import nat  # noqa: F401 (fixture)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batch_util as bu  # noqa: E402
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

POINT_BOUND, CAR_BOUND = 0.15811388, 0.21569655   # bounding radius of the robots (shape_bound)
MIN_REACH = 0.005                                 # the classification's reach is never below its constant term
SQRT2 = 1.4142135


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _assert_bits(a, b, what):
  np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
def test_every_record_float_round_trips(nat, robot):
  """set_state with a distinct finite value in every float of every env, get_state returns it bit for bit."""
  n = 67
  rf, ri = bu.sample_records_native(robot, 'go_to_goal', n, seed=31)
  ctx = nat.Context(robot, n, seed=31)
  ctx.set_layout(rf, ri)
  _, ri0 = ctx.get_state()
  k, e = np.meshgrid(np.arange(nat.REC_FLOATS), np.arange(n))
  want = (1.0 + k + e / 128.0).astype(np.float32)        # exact in fp32, different for every (field, env)
  assert len(np.unique(want)) == want.size
  ctx.set_state(want, ri0)
  got, ri1 = ctx.get_state()
  _assert_bits(got, want, 'record floats after set_state / get_state')
  ctx.set_state(got, ri1)
  got2, ri2 = ctx.get_state()
  _assert_bits(got2, want, 'second round trip')
  np.testing.assert_array_equal(ri2, ri1)
  counts = [nat.I_TASK, nat.I_NH, nat.I_NV, nat.I_NP, nat.I_NB, nat.I_BOX_KIND, nat.I_STEP, nat.I_ENV_ID]
  np.testing.assert_array_equal(ri1[:, counts], ri0[:, counts])
  ctx.close()


def _place(nat, run, bound, gap_lo):
  """Robots where the classification has to decide.  Env 3 j: beside its first vase (along +x, heading away), the vase's
  yaw swept over [0, pi / 2) and the gap between the vase's face and the robot's centre from gap_lo (the footprint test
  fires at any yaw) to just inside the bounding circle (it fires at no yaw).  Env 6 j + 1: on its goal (the task object
  instead, where there is one), so the goal is met in step 1.  Env 6 j + 4: in front of its first vase, outside the
  circle, moving towards it: quiet at first, busy some steps later.  -> (ids beside a vase, record floats as set)."""
  ctx = run.ctx
  rf, ri = ctx.get_state()
  n = len(rf)
  env = np.arange(n)
  has_v = ri[:, nat.I_NV] > 0
  vsz = rf[:, nat.F_VASE_SIZE]
  beside = env[(env % 3 == 0) & has_v]
  j = np.arange(len(beside))
  frac = lambda x: x - np.floor(x)   # noqa: E731
  gap_hi = bound + MIN_REACH + (SQRT2 - 1) * vsz[beside] - 0.004
  gap = gap_lo + (gap_hi - gap_lo) * frac(j * 0.7548777)
  rf[beside, nat.F_VASES + 2] = (frac(j * 0.3819660) * np.pi / 2).astype(np.float32)
  rf[beside, nat.F_ROBOT] = rf[beside, nat.F_VASES] + vsz[beside] + gap.astype(np.float32)
  rf[beside, nat.F_ROBOT + 1] = rf[beside, nat.F_VASES + 1]
  rf[beside, nat.F_ROBOT + 2:nat.F_ROBOT + 6] = 0
  on_goal = env[env % 6 == 1]
  who = nat.F_BOX if (ri[:, nat.I_BOX_KIND] > 0).any() else nat.F_ROBOT
  rf[on_goal, who] = rf[on_goal, nat.F_GOAL]
  rf[on_goal, who + 1] = rf[on_goal, nat.F_GOAL + 1]
  comer = env[(env % 6 == 4) & has_v]
  j = np.arange(len(comer))
  dist = bound + MIN_REACH + SQRT2 * vsz[comer] + 0.03 + 0.008 * j
  rf[comer, nat.F_ROBOT] = rf[comer, nat.F_VASES] - dist.astype(np.float32)
  rf[comer, nat.F_ROBOT + 1] = rf[comer, nat.F_VASES + 1]
  rf[comer, nat.F_ROBOT + 2] = 0
  rf[comer, nat.F_ROBOT + 3] = 0.6
  rf[comer, nat.F_ROBOT + 4:nat.F_ROBOT + 6] = 0
  ctx.set_state(rf, ri)
  return beside, rf


def _inside_circle(nat, rf, ri, bound):
  """Envs with a vase inside the smallest bounding circle the classification can use (reach >= MIN_REACH): all of them
  are busy by circles alone."""
  hit = np.zeros(len(rf), bool)
  for k in range(nat.MAX_VASES):
    d = np.hypot(rf[:, nat.F_VASES + 6 * k] - rf[:, nat.F_ROBOT], rf[:, nat.F_VASES + 6 * k + 1] - rf[:, nat.F_ROBOT + 1])
    hit |= (k < ri[:, nat.I_NV]) & (d <= bound + MIN_REACH + SQRT2 * rf[:, nat.F_VASE_SIZE] - 1e-4)
  return hit


def _lockstep(nat, monkeypatch, robot, task, n, steps, bound, gap_lo):
  """Split and single form from the same placed state, compared bit for bit after every step -> per step of the split
  run: busy count, envs inside a bounding circle before the step, and the goals before / after step 1."""
  runs = []
  for split in ('1', '0'):
    monkeypatch.setenv('SAG_SPLIT', split)
    runs.append(bench.DeviceRun(task, n, 0, 0, robot=robot))
  states = [_place(nat, r, bound, gap_lo)[1] for r in runs]
  _assert_bits(states[0], states[1], 'placed state')
  goal0 = states[0][:, nat.F_GOAL:nat.F_GOAL + 2].copy()
  busy, circ, goal1 = [], [], None
  for t in range(steps):
    rf, ri = runs[0].ctx.get_state()
    circ.append(int(_inside_circle(nat, rf, ri, bound).sum()))
    for r in runs:
      r.step()
    a, b = runs[0].outputs(), runs[1].outputs()
    for name in ('obs', 'reward', 'cost', 'done', 'goal_met'):
      _assert_bits(a[name], b[name], f'{name}, step {t + 1}')
    (fa, ia), (fb, ib) = runs[0].ctx.get_state(), runs[1].ctx.get_state()
    _assert_bits(fa, fb, f'state floats, step {t + 1}')
    np.testing.assert_array_equal(ia, ib, err_msg=f'state ints, step {t + 1}')
    busy.append(runs[0].ctx.busy_count())
    assert runs[1].ctx.busy_count() == 0, 'the single launch keeps no busy list'
    if t == 0:
      goal1 = fa[:, nat.F_GOAL:nat.F_GOAL + 2].copy()
  for r in runs:
    r.close()
  return busy, circ, goal0, goal1


def test_lazy_yaw_decides_as_the_single_launch(nat, monkeypatch):
  """Point / go_to_goal, 193 envs, 30 steps.  The split run must have used both launches, turned a quiet env busy (its hot
  record then comes from the quiet kernel, yaw included), kept envs quiet that circles alone would call busy, and moved a
  goal in step 1."""
  n = 193
  busy, circ, goal0, goal1 = _lockstep(nat, monkeypatch, 'point', 'go_to_goal', n, 30, POINT_BOUND, 0.10)
  print('busy per step', busy, 'inside a bounding circle before the step', circ)
  assert any(0 < b < n for b in busy), busy
  assert any(b1 > b0 for b0, b1 in zip(busy[1:], busy[2:])), f'no quiet env ever turned busy: {busy}'
  # the busy launch of step t + 1 runs the envs classified at the end of step t, i.e. from the state before step t + 1
  assert any(b < c for b, c in zip(busy[1:], circ[1:])), f'the footprint test never kept an env quiet: {busy} vs {circ}'
  assert (_bits(goal0) != _bits(goal1)).any(), 'no goal moved in step 1'


def test_car_push_box_split_equals_single(nat, monkeypatch):
  """Car / push_box, 65 envs, 20 steps: the quiet Car kernel reads no yaw at all."""
  n = 65
  busy, _, goal0, goal1 = _lockstep(nat, monkeypatch, 'car', 'push_box', n, 20, CAR_BOUND, 0.16)
  print('busy per step', busy)
  assert any(0 < b < n for b in busy), busy


def test_failed_env_keeps_goal_and_last(nat, monkeypatch):
  """A non-finite robot velocity: done, and neither the goal nor the last goal distance of that env is stored - in the
  busy launch (first step after set_state) and in the quiet one (second step); all other envs equal the single launch."""
  n, sick = 65, [3, 64]
  ctxs = []
  rf, ri = bu.sample_records('point', 'go_to_goal', n)
  for split in ('1', '0'):
    monkeypatch.setenv('SAG_SPLIT', split)
    c = nat.Context('point', n, seed=12)
    c.set_layout(rf, ri)
    s_rf, s_ri = c.get_state()
    s_rf[sick[0], nat.F_ROBOT + 3] = np.nan
    s_rf[sick[1], nat.F_ROBOT + 4] = np.inf
    c.set_state(s_rf, s_ri)
    ctxs.append(c)
  keep = [nat.F_GOAL, nat.F_GOAL + 1, nat.F_LAST]
  before = ctxs[0].get_state()[0][np.ix_(sick, keep)]
  act = np.full((n, 2), 0.5, np.float32)
  for t in range(2):
    outs = [c.step(act) for c in ctxs]
    (fa, ia), (fb, ib) = ctxs[0].get_state(), ctxs[1].get_state()
    for f, o in ((fa, outs[0]), (fb, outs[1])):
      _assert_bits(f[np.ix_(sick, keep)], before, f'goal and last0 of the failed envs, step {t + 1}')
      assert o[3][sick].all() and o[3].sum() == len(sick), f'done, step {t + 1}'
    ok = np.ones(n, bool)
    ok[sick] = False
    for x, y in zip(outs[0][:5], outs[1][:5]):
      _assert_bits(x[ok], y[ok], f'outputs of the healthy envs, step {t + 1}')
    _assert_bits(fa[ok], fb[ok], f'state of the healthy envs, step {t + 1}')
    np.testing.assert_array_equal(ia[ok], ib[ok])
  assert 0 <= ctxs[0].busy_count() < n
  for c in ctxs:
    c.close()

"""Directed contact-branch tests: the device narrow phase (csrc/sag_device.hpp: cc_contact, cb_contact with its
centre-inside-the-box branch, bb_contact / verts_inside_mask / vert_contact, boxes_separated, the pair masks of
collide_list_nb<SHA, 1> and <SHA, 5> with the Car's 64-bit mask, the ball's presented radius, the Dyn pool with its
overflow path, the sleep / wake walk order) against both builds of the oracle, on states in which overlaps are the rule.
The tenth case, Car / dribble_ball, is a finding of the others: the oracle's sphere-and-arrow treatment of the ball also took
the Car (95 of 576 rows off on the host build of the device sources) and is now the Point's alone, as in the kernels.

contact_ref.directed_records places every body of an env around its robot; contact_ref.census (a float64 restatement of
the footprints and pair tests, pinned by tests/test_contact_ref.py) says which branches the states reach, and
contact_ref.reach states what each case must reach: every row is asserted over the states the steps started from.  The
census is never the expected value of a step - that is the oracle's.

Each case: 192 envs x 3 steps, resynchronised from the device every step as the lockstep of tests/test_gpu_parity.py, zero
action noise, the lockstep's random tape (read only where a task draws: a goal resample, a goal button), uniform random
actions.  Per step
  * launch forms: contexts made under SAG_SPLIT=1 and under SAG_SPLIT=1, SAG_BUSY_KINDS=1, SAG_BUSY_KINDS_MIN=0 are stepped
    with the same inputs; outputs and state are bit-equal to the single launch (after an install every env is busy);
  * state against the fp64 and the fp32 oracle within the lockstep's tolerances (batch_util.lockstep_state_tol); rows
    outside are counted, not hidden;
  * done, goal_met, words used and the task ints equal the fp64 oracle's on EVERY row - the state check masks nothing -
    except on a row where the two oracle builds disagree in one of them: there the device equals one of the two;
  * cost flags exact unless the oracle reports the decision within 1e-5 of its threshold or, a contact whose penetration
    changes sign with the arithmetic, the fp32 oracle sides with the device (the lockstep's rule);
  * reward within 2e-4 on rows inside the state tolerance.

Rows outside the state tolerance are budgeted at 2 x measured + 2 (the counts are single digits: a pure ratio would flap
on one contact onset).  MEASURED holds, per case, the rows out of 576 on the MI355X: (device vs fp64 oracle, device vs
fp32 oracle, fp32 oracle vs fp64 oracle) - the last is the yardstick, the reference's own precision on these states.
Whatever is measured, no case may leave more than 5 % of its env-steps outside the tolerance, the oracle builds may
disagree on at most 2 %, and discrete exceptions (rows excused by the oracle builds' disagreement, cost flags at a
threshold) apply to at most 1 %: inputs that break these are to be changed, not budgeted.
Measured (rows of 576; discrete exceptions and cost flags at a threshold: 0 in every case):
  case             device vs fp64   device vs fp32   fp32 oracle vs fp64 oracle
  vase_crowd             0                0                 0
  wake_order             0                0                 0
  buttons                0                0                 0
  push_box               0                0                 0
  roll_rod               1                0                 1
  dribble_ball           0                0                 0
  point_haul_box         0                0                 0
  car_haul_box           0                1                 1
  car_push_box           1                2                 1
  car_dribble_ball       3                3                 1
The lines of that run, with what every case reached, are kept in profiles/contact_branches_counts.txt."""
import os

import numpy as np
import pytest

import batch_util as bu
import contact_ref as cr
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

N_ENVS, N_STEPS = 192, 3   # the smallest size at which every row of contact_ref.reach still occurred >= 5 times

# rows of 576 outside the state tolerance on the MI355X: device vs fp64, device vs fp32, fp32 oracle vs fp64 oracle
MEASURED = {
    'vase_crowd': (0, 0, 0),
    'wake_order': (0, 0, 0),
    'buttons': (0, 0, 0),
    'push_box': (0, 0, 0),
    'roll_rod': (1, 0, 1),
    'dribble_ball': (0, 0, 0),
    'point_haul_box': (0, 0, 0),
    'car_haul_box': (0, 1, 1),
    'car_push_box': (1, 2, 1),
    'car_dribble_ball': (3, 3, 1),
}

LOG_DIR_ENV = 'SAG_CONTACT_LOG_DIR'   # a directory: the lines are appended to contact_branches_counts.txt there (unset: printed only)


def _log(line):
  print(line)
  if os.environ.get(LOG_DIR_ENV):
    os.makedirs(os.environ[LOG_DIR_ENV], exist_ok=True)
    with open(os.path.join(os.environ[LOG_DIR_ENV], 'contact_branches_counts.txt'), 'a') as f:
      f.write(line + '\n')


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def oracle():
  return Oracle()


@pytest.fixture(scope='module')
def oracle32():
  return Oracle(f32=True)


def _contexts(nat, monkeypatch, robot, rf, ri, awake):
  """The single launch, the split launch and the split launch with the busy list kept by kind of contact, each with the
  directed state installed (set_layout, then the case's awake word through get_state / set_state)."""
  ctxs = []
  for flag, kinds_min in (('0', None), ('1', None), ('1', '0')):
    monkeypatch.setenv('SAG_SPLIT', flag)
    if kinds_min is None:
      monkeypatch.delenv('SAG_BUSY_KINDS_MIN', raising=False)
      monkeypatch.delenv('SAG_BUSY_KINDS', raising=False)
    else:
      monkeypatch.setenv('SAG_BUSY_KINDS_MIN', kinds_min)
      monkeypatch.setenv('SAG_BUSY_KINDS', '1')     # (the default keeps kinds for the Car only)
    c = nat.Context(robot, len(rf), seed=1234)
    c.set_layout(rf, ri)
    s_rf, s_ri = c.get_state()
    s_ri[:, nat.I_AWAKE] = awake
    c.set_state(s_rf, s_ri)
    ctxs.append(c)
  monkeypatch.delenv('SAG_BUSY_KINDS_MIN', raising=False)
  monkeypatch.delenv('SAG_BUSY_KINDS', raising=False)
  return ctxs


@pytest.mark.parametrize('name', list(cr.CASES))
def test_contact_branches(nat, oracle, oracle32, monkeypatch, name):
  robot, task = cr.CASES[name][:2]
  n, T = N_ENVS, N_STEPS
  rid = {'point': 0, 'car': 1}[robot]
  od = 60 if robot == 'point' else 72
  base = bu.sample_records_native(robot, task, n, seed=cr.CASE_SEED[name])
  rf, ri, awake = cr.directed_records(name, n, base)
  ctxs = _contexts(nat, monkeypatch, robot, rf, ri, awake)
  rng = np.random.RandomState(cr.CASE_SEED[name] + 1)
  noise = np.zeros((n, 2), np.float32)
  tally = cr.Tally()
  viol64 = viol32 = viol_oo = excused = n_near = n_cost = n_wrong = n_wrong_cost = n_wrong_rew = 0
  off, problems = [], []   # rows outside the state tolerance; (problems are asserted after the counts are logged: a failure then comes with its figures)
  min_dynamic = chain_envs = taut_envs = slack_envs = None
  events = np.zeros(n, bool)
  for t in range(T):
    rf, ri = ctxs[0].get_state()
    cen = [cr.census(rf[e], ri[e], robot) for e in range(n)]
    for c in cen:
      tally.add(c.overlaps)
    if t == 0:
      if awake == 0:   # (a body in motion is awake by its velocity: the word a state exports names resting bodies only)
        assert not ri[:, nat.I_AWAKE].any()
      min_dynamic = min(c.n_dynamic for c in cen)
      chain_envs = sum(bool(cr.wake_chains(rf[e], ri[e], robot, cen[e].overlaps)) for e in range(n))
      taut_envs, slack_envs = sum(c.taut is True for c in cen), sum(c.taut is False for c in cen)
    arr, arr32 = oracle.make_batch(rf, ri), oracle32.make_batch(rf, ri)
    act = rng.uniform(-1, 1, (n, 2)).astype(np.float32) * (0.04 if robot == 'car' else 1.0)   # (car.xml:7: |u| >= .02 saturates)
    tape = rng.randint(0, 2**32, size=(n, 64), dtype=np.uint32)
    outs = [c.step(act, noise, tape) for c in ctxs]
    _, d_rew, d_cost, d_done, d_met, d_used = outs[0]
    d_rf, d_ri = ctxs[0].get_state()
    # launch forms
    if t == 0:
      assert ctxs[1].busy_count() == n and ctxs[2].busy_count() == n, 'after an install every env is busy'
    for form, (other, c) in enumerate(zip(outs[1:], ctxs[1:]), 1):
      for a, b in zip(outs[0], other):
        np.testing.assert_array_equal(a, b, err_msg=f'launch form {form} step {t}')
      s_rf, s_ri = c.get_state()
      np.testing.assert_array_equal(d_rf, s_rf, err_msg=f'launch form {form} state step {t}')
      np.testing.assert_array_equal(d_ri, s_ri, err_msg=f'launch form {form} ints step {t}')
    # the two oracle builds
    _, o_rew, o_cost, o_done, o_met, o_used, o_margin = oracle.step_batch_full(arr, rid, act, noise, tape, obs_dim=od)
    _, _, p_cost, p_done, p_met, p_used, _ = oracle32.step_batch_full(arr32, rid, act, noise, tape, obs_dim=od)
    o_rf, o_ri = oracle.batch_records(arr)
    p_rf, p_ri = oracle32.batch_records(arr32)
    tol64, tol32 = bu.lockstep_state_tol(robot, task, d_rf.shape[1])
    bad64, bad32 = bu.rows_outside(d_rf, o_rf, tol64), bu.rows_outside(d_rf, p_rf, tol32)
    viol64 += int(bad64.sum()); viol32 += int(bad32.sum())
    viol_oo += int(bu.rows_outside(p_rf, o_rf, tol64).sum())
    for e in np.flatnonzero(bad64 | bad32)[:2]:   # (the census names the branches to look at)
      off.append(f'step {t} env {e} (fp64 {bool(bad64[e])}, fp32 {bool(bad32[e])}): {_census_keys(cen[e])}')
    # discrete outputs on every row
    disc = lambda done, met, used, ints: np.concatenate([done[:, None], met[:, None], used[:, None], ints], 1).astype(np.int64)   # noqa: E731
    dd, do, dp = disc(d_done, d_met, d_used, d_ri), disc(o_done, o_met, o_used, o_ri), disc(p_done, p_met, p_used, p_ri)
    eq64, eq32, builds_agree = (dd == do).all(1), (dd == dp).all(1), (do == dp).all(1)
    wrong = ~eq64 & (builds_agree | ~eq32)
    if wrong.any():
      problems.append(f'step {t}: discrete outputs (done, goal_met, words used, task ints) differ from the fp64 oracle in envs '
                             f'{np.flatnonzero(wrong)[:8]}: device {dd[wrong][:2]}, fp64 {do[wrong][:2]}, fp32 {dp[wrong][:2]}; '
                             f'census of the first: {_census_keys(cen[int(np.flatnonzero(wrong)[0])])}')
    n_wrong += int(wrong.sum())
    excused += int((~eq64 & ~wrong).sum())
    # cost flags
    differ = d_cost != o_cost
    mism = differ & (o_margin > 1e-5) & (d_cost != p_cost)   # (away from a threshold the fp32 oracle must side with the device)
    if mism.any():
      problems.append(f'cost flag mismatch away from any threshold at step {t}: envs {np.flatnonzero(mism)[:8]}')
    n_wrong_cost += int(mism.sum())
    n_near += int((differ & ~mism).sum())
    n_cost += int(o_cost.sum())
    ok = ~bad64
    rew_off = ok & (np.abs(d_rew - o_rew) > 2e-4).any(1)
    if rew_off.any():
      problems.append(f'reward step {t}: envs {np.flatnonzero(rew_off)[:8]} differ by up to {np.abs(d_rew - o_rew)[rew_off].max():.3g} on rows inside the state tolerance')
    n_wrong_rew += int(rew_off.sum())
    events |= (d_met != 0) | (d_ri[:, nat.I_BTN_STATE] != ri[:, nat.I_BTN_STATE])
  for c in ctxs:
    c.close()

  # what the states reached
  rows = cr.reach(name, tally)
  if name == 'vase_crowd':
    rows.append(('dynamic free bodies in the env that has fewest (DPOOL = 3: 4 overflow the pool)', min_dynamic, min_dynamic, 4))
  if name == 'wake_order':
    rows.append(('envs: a moving vase on a sleeper that lies on another sleeper', chain_envs, chain_envs, 20))
  if name == 'buttons':
    rows.append(('envs whose button contacts changed I_BTN_STATE or met the goal', int(events.sum()), int(events.sum()), 10))
  if task == 'haul_box':
    rows.append(('envs with the box beyond the tether\'s range', taut_envs, taut_envs, 20))
    rows.append(('envs with the box within the tether\'s range', slack_envs, slack_envs, 20))
  steps = n * T
  m64, m32, moo = MEASURED[name]
  _log(f'{name} ({robot} / {task}): {n} envs x {T} steps | rows outside the state tolerance: device vs fp64 oracle {viol64}, device vs fp32 '
       f'oracle {viol32}, fp32 oracle vs fp64 oracle {viol_oo} (budgets {2 * m64 + 2} / {2 * m32 + 2}) | discrete rows excused by the oracle '
       f'builds\' disagreement {excused}, cost flags within 1e-5 of a threshold {n_near} | oracle cost flag up in {n_cost} env-steps | rows WRONG: '
       f'discrete {n_wrong}, cost flag {n_wrong_cost}, reward {n_wrong_rew}')
  for what, cnt, deep, minimum in rows:
    _log(f'    {what}: {cnt} ({deep} deeper than 1 mm), needs >= {minimum}')
  for line in off[:6]:
    _log(f'    outside the state tolerance, {line}')
  assert not problems, problems[:4]
  missed = [r for r in rows if r[1] < r[3]]
  assert not missed, f'the states of {name} do not reach: {missed}'
  assert n_cost >= 0.5 * steps, 'the crowd should be in contact with the robot in most env-steps'
  assert viol_oo <= 0.02 * steps, f'the oracle builds disagree on {viol_oo} rows'
  assert max(viol64, viol32) <= 0.05 * steps, f'{viol64} / {viol32} rows outside the fp64 / fp32 tolerance'
  assert excused + n_near <= 0.01 * steps, f'{excused} + {n_near} discrete exceptions'
  assert viol64 <= 2 * m64 + 2, f'{viol64} rows outside the fp64 tolerance, measured {m64}'
  assert viol32 <= 2 * m32 + 2, f'{viol32} rows outside the fp32 tolerance, measured {m32}'


def _census_keys(census):
  """The census keys of one env, for a failure message: the branch names what to look at."""
  return sorted({o.key + (o.verts,) for o in census.overlaps if o.depth > 0}, key=str)

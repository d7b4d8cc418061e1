"""The census of tests/doggo_branch_ref.py pinned on paper and against the oracle's own row count, and every case of
tests/test_doggo_branches.py shown to reach its table with the oracle alone (no device): the fp64 oracle's own rollout of
the case, with the actions and the tape of the GPU test, resynchronised through fp32 records every step as there."""
import ctypes as C
import time

import numpy as np
import pytest

import batch_util as bu
import doggo_branch_ref as dbr
import oracle_lib as ol
from oracle_lib import Oracle
from test_oracle_doggo import ANKLE_1, TORSO_FRONT, TORSO_REAR, VASE0, contact_scenarios, doggo_record

EXT = dbr.EXT


@pytest.fixture(scope='module')
def oracle():
  return Oracle()


@pytest.fixture(scope='module')
def oracle32():
  return Oracle(f32=True)


@pytest.fixture(scope='module')
def settled(oracle):
  return dbr.settled_pose(oracle)


def case_records(name, oracle, settled, n=dbr.N_ENVS):
  base = bu.sample_records_native('doggo', dbr.CASES_ALL[name]['task'], n, seed=dbr.CASE_SEED[name])
  return dbr.directed_records(name, n, base, oracle, settled)


def row_hist(oracle, reset=True):
  hist = (C.c_long * 99)()
  oracle.lib.sago_doggo_row_hist(hist, 1 if reset else 0)
  return np.array(list(hist))


def test_settled_pose_rests_on_18_rows(oracle, settled):
  """Eight zero-action steps from the reset pose: z .2034 -> .1649, on 6 joint limits and 4 feet."""
  rf, ri = doggo_record()
  assert settled[EXT] == pytest.approx(0.1649, abs=5e-4)
  assert np.abs(settled[EXT + 5:EXT + 9]).max() < 0.05 and abs(settled[3]) < 0.05 and abs(settled[4]) < 0.05
  rf[0:6], rf[EXT:EXT + 35] = settled[0:6], settled[EXT:EXT + 35]
  c = dbr.census(oracle, rf, ri)
  assert c.lower + c.upper == 6 and sorted(c.floor) == list(dbr.FOOT_POINTS) and not c.objects
  assert c.rows == 18 and c.path == 'fast' and c.taut is None


def test_census_of_the_analytic_scenarios(oracle):
  sc = contact_scenarios()
  c = dbr.census(oracle, *sc['vase corner 5 mm inside the shaft of ankle_1'][:2])
  assert len(c.objects) == 1 and c.rows == 3 and c.path == 'fast' and c.cost_contacts == 1
  o = c.objects[0]
  assert (o.cls, o.obj, o.g, o.robot_kind, o.obj_kind) == ('vase', VASE0, ANKLE_1, 'capsule', 'box')
  assert o.depth == pytest.approx(0.005, abs=1e-6) and o.site is None and not o.crosses and not o.above   # 3/4 down the shaft: in neither site
  assert dbr.census(oracle, *sc['the same vase 1 cm further out'][:2]).rows == 0
  c = dbr.census(oracle, *sc['pillar 3 mm inside the shafts of hip_1 and ankle_1'][:2])
  assert [(o.cls, o.obj_kind) for o in c.objects] == [('pillar', 'circle')] * 2 and c.rows == 6
  assert [o.crosses or o.above for o in c.objects] == [False, False]                    # a pillar is 1 m tall
  c = dbr.census(oracle, *sc['vase face 4 mm inside the torso cylinders at the waist'][:2])
  assert len(c.objects) == 6 and c.rows == 18
  torso = [o for o in c.objects if o.g in (TORSO_FRONT, TORSO_REAR)]
  assert len(torso) == 4 and all(o.robot_kind == 'cylinder' and o.above and not o.crosses for o in torso)   # the axis (z .22) is above the vase's top (.2)
  c = dbr.census(oracle, *sc['lying on its left side on the knees of legs 1 and 2'][:2])
  assert sorted(c.floor) == [3, 11] and set(c.floor) <= set(dbr.KNEE_POINTS) and c.rows == 6


def test_census_counts_joints_beyond_their_range_and_the_tether(oracle):
  rf, ri = doggo_record(z=5.0)
  lo, hi = dbr.joint_range()
  assert dbr.census(oracle, rf, ri).rows == 0                       # joints at 0: on the bounds of 6 ranges, beyond none
  rf[EXT + 9 + 1] = lo[1] - 0.01                                    # hip_1_y below -75 degrees
  rf[EXT + 9 + 8] = hi[8] + 0.01                                    # hip_2_y above 135 degrees
  c = dbr.census(oracle, rf, ri)
  assert (c.lower, c.upper, c.rows) == (1, 1, 2)
  # the tether: base site (z .2034) <-> box site (z .2)
  for d, taut in ((0.74, False), (0.76, True)):
    rf, ri = doggo_record(z=0.2034, task='haul_box', names=('robot', 'goal'))
    ri[ol.I_BOX_KIND] = 1
    rf[ol.F_BOX:ol.F_BOX + 2] = [d, 0.0]
    c = dbr.census(oracle, rf, ri)
    assert c.taut is taut and c.rows == int(taut)
  # at the heights involved: from the settled base (z .165) the box site is .035 higher, .7492^2 + .035^2 < .75^2 < .7493^2 + .035^2
  for d, taut in ((0.7491, False), (0.7493, True)):
    rf, ri = doggo_record(z=0.165, task='haul_box', names=('robot', 'goal'))
    ri[ol.I_BOX_KIND] = 1
    rf[ol.F_BOX:ol.F_BOX + 2] = [0.0, -d]
    assert dbr.census(oracle, rf, ri).taut is taut


def test_census_rows_equal_the_oracles_row_histogram(oracle, settled):
  """One nstep = 0 evaluation of a directed state increments exactly the bin the census names (states of five cases, the
  overflow case among them: 100 in all)."""
  seen = set()
  n_states = 0
  for name in ('torso_vases', 'pillars', 'haul_box', 'joint_limits', dbr.OVERFLOW):
    rf, ri = case_records(name, oracle, settled, 20)
    for e in range(20):
      c = dbr.census(oracle, rf[e], ri[e])
      row_hist(oracle)
      oracle.step(oracle.env(rf[e], ri[e]), dbr.DOGGO, np.zeros(12), noise=np.zeros(12), nstep=0)
      h = row_hist(oracle)
      assert h.sum() >= 1 and h[c.rows] == h.sum(), (name, e, c.rows, np.flatnonzero(h))
      seen.add(c.path)
      n_states += 1
  assert n_states >= 64 and seen == {'fast', 'wide', 'overflow'}


def test_every_branch_is_in_some_case():
  named = {k for spec in dbr.CASES.values() for k in spec['reach']}
  want = (set(dbr.ROWS) - {'box', 'button_event'}) | {'box', 'rod', 'ball', 'press_event', 'collect_event'}
  assert want <= named, want - named
  assert dbr.CASES['press_buttons']['task'] == 'press_buttons' and dbr.CASES['collect']['task'] == 'collect'
  assert dbr.CASES['roll_rod']['task'] == 'roll_rod' and dbr.CASES['dribble_ball']['task'] == 'dribble_ball'


def oracle_rollout(name, oracle, oracle32, settled):
  """The fp64 oracle's own rollout of a case: (tally, figures)."""
  n, T = dbr.N_ENVS, dbr.N_STEPS
  rf, ri = case_records(name, oracle, settled)
  rng = np.random.RandomState(dbr.CASE_SEED[name] + 1)
  tally = dbr.Tally()
  after = any(k in dbr.CASES[name]['reach'] for k in ('after_vase', 'after_static', 'after_object', 'sleeper'))
  tol = bu.doggo_state_tol(rf.shape[1])
  fig = dict(viol_oo=0, disagree=0, near=0, cost=0, hist=np.zeros(99, np.int64))
  for t in range(T):
    cen = [dbr.census(oracle, rf[e], ri[e]) for e in range(n)]
    tally.add(t, cen, rf, ri, after)
    arr, arr32 = oracle.make_batch(rf, ri), oracle32.make_batch(rf, ri)
    act, noise, tape = dbr.step_inputs(rng, n)
    row_hist(oracle)
    _, _, o_cost, o_done, o_met, o_used, o_margin = oracle.step_batch_full(arr, 2, act, noise, tape, obs_dim=104)
    fig['hist'] += row_hist(oracle)
    _, _, p_cost, p_done, p_met, p_used, _ = oracle32.step_batch_full(arr32, 2, act, noise, tape, obs_dim=104)
    o_rf, o_ri = oracle.batch_records(arr)
    p_rf, p_ri = oracle32.batch_records(arr32)
    fig['viol_oo'] += int(bu.rows_outside(p_rf, o_rf, tol).sum())
    fig['disagree'] += int((dbr.discrete(o_done, o_met, o_used, o_ri) != dbr.discrete(p_done, p_met, p_used, p_ri)).any(1).sum())
    fig['near'] += int(((o_cost != p_cost) & (o_margin <= 1e-5)).sum())
    fig['cost'] += int(o_cost.sum())
    tally.events += int(dbr.button_events(ri, o_ri, o_met).sum())
    assert np.isfinite(o_rf).all() and not o_done.any()
    rf, ri = o_rf, o_ri
  return tally, fig


@pytest.mark.parametrize('name', list(dbr.CASES))
def test_case_reaches_its_table_with_the_oracle_alone(oracle, oracle32, settled, name):
  t0 = time.time()
  tally, fig = oracle_rollout(name, oracle, oracle32, settled)
  steps = dbr.N_ENVS * dbr.N_STEPS
  rows = dbr.reach(name, tally)
  hist = np.flatnonzero(fig['hist'])
  print(f'{name}: {dbr.N_ENVS} envs x {dbr.N_STEPS} steps, oracle alone ({time.time() - t0:.1f} s) | fp32 oracle vs fp64 oracle outside the state '
        f'tolerance {fig["viol_oo"]} | rows on which the builds\' discrete outputs differ {fig["disagree"]}, cost flags within 1e-5 of a threshold '
        f'{fig["near"]} | cost flag up in {fig["cost"]} env-steps | rows per evaluation {hist.min()} - {hist.max()}')
  for what, cnt, minimum in rows:
    print(f'    {what}: {cnt}, needs >= {minimum}')
  missed = [r for r in rows if r[1] < r[2]]
  assert not missed, f'the states of {name} do not reach: {missed}'
  assert fig['viol_oo'] <= 0.02 * steps, f'the oracle builds disagree in state on {fig["viol_oo"]} rows'              # condition 2
  assert fig['disagree'] + fig['near'] <= 0.01 * steps, f'{fig["disagree"]} + {fig["near"]} discrete exceptions'      # condition 3
  assert hist.max() <= dbr.ROW_BUDGET, f'an evaluation of the oracle had {hist.max()} rows'                          # condition 4


def test_overflow_case_straddles_the_row_budget(oracle, settled):
  rf, ri = case_records(dbr.OVERFLOW, oracle, settled)
  cen = [dbr.census(oracle, rf[e], ri[e]) for e in range(len(rf))]
  rows = np.array([c.rows for c in cen])
  contacts = np.array([len(c.objects) for c in cen])
  assert rows.min() >= 45 and rows.max() <= 60 and contacts.min() >= 9 and contacts.max() <= 14
  assert (rows > dbr.ROW_BUDGET).sum() >= 10 and (rows <= dbr.ROW_BUDGET).sum() >= 10
  assert sum(c.taut is True for c in cen) >= 10 and sum(c.taut is False for c in cen) >= 10
  # both sides of the tether's row at the budget: 50 rows and slack (nothing to drop); 50 rows, then the taut tether's (the one dropped)
  assert sum(c.rows == dbr.ROW_BUDGET and c.taut is False for c in cen) >= 5
  assert sum(c.rows == dbr.ROW_BUDGET + 1 and c.taut is True and c.lower + c.upper == 8 for c in cen) >= 5

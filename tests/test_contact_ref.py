"""The census of tests/contact_ref.py on poses whose branch and depth are known on paper, and the case table of
tests/test_contact_branches.py on the states its cases install (the census needs no GPU: the GPU test asserts the same
table over the states its steps really started from)."""
import math

import numpy as np
import pytest

import batch_util as bu
import contact_ref as cr
from oracle_lib import (F_BOX, F_BUTTONS, F_PILLAR_SIZE, F_PILLARS, F_ROBOT, F_VASE_SIZE, F_VASES, I_AWAKE, I_BOX_KIND,
                        I_NB, I_NP, I_NV, I_TASK, REC_FLOATS, REC_INTS)


def _hit(got, branch, depth, verts=None):
  assert got is not None and got[0] == branch and got[1] == verts, got
  assert got[2] == pytest.approx(depth, abs=1e-12), got


def test_circle_circle_on_paper():
  _hit(cr.circle_circle(0, 0, 0.1, 0.25, 0, 0.2), 'cc', 0.05)
  _hit(cr.circle_circle(1, 1, 0.1, 1.03, 1.04, 0.05), 'cc', 0.1)          # a 3-4-5 triangle: distance .05
  assert cr.circle_circle(0, 0, 0.125, 0.375, 0, 0.25) is None              # touching is not a contact (binary fractions: exact)
  assert cr.circle_circle(0, 0, 0.1, 0.31, 0, 0.2) is None


def test_circle_box_on_paper():
  # box of half (.2, .1) at the origin, unrotated
  _hit(cr.circle_box(0.25, 0.0, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-face', 0.05)
  _hit(cr.circle_box(0.0, -0.15, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-face', 0.05)
  _hit(cr.circle_box(0.23, 0.14, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-corner', 0.05)   # (.03, .04) off the corner
  assert cr.circle_box(0.34375, 0.25, 0.15625, 0, 0, 0, 0.25, 0.125) is None    # (3, 4) / 32 off the corner, radius 5 / 32: touching, exact
  _hit(cr.circle_box(0.34375, 0.25, 0.1875, 0, 0, 0, 0.25, 0.125), 'cb-corner', 0.03125)
  assert cr.circle_box(0.375, 0.0, 0.125, 0, 0, 0, 0.25, 0.125) is None         # touching a face
  # the centre inside: the nearer face expels it, depth = radius + distance to that face
  _hit(cr.circle_box(0.17, 0.0, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-centre-inside', 0.13)   # x face at .03, y faces at .1
  _hit(cr.circle_box(0.05, 0.08, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-centre-inside', 0.12)  # y face at .02, x face at .15
  _hit(cr.circle_box(0.2, 0.0, 0.1, 0, 0, 0, 0.2, 0.1), 'cb-centre-inside', 0.1)     # on the boundary
  # the same box turned by 90 degrees about (1, 2): its long side now lies along y
  _hit(cr.circle_box(1.0, 2.25, 0.1, 1, 2, math.pi / 2, 0.2, 0.1), 'cb-face', 0.05)
  _hit(cr.circle_box(1.15, 2.0, 0.1, 1, 2, math.pi / 2, 0.2, 0.1), 'cb-face', 0.05)
  _hit(cr.circle_box(1.0, 2.17, 0.1, 1, 2, math.pi / 2, 0.2, 0.1), 'cb-centre-inside', 0.13)


def test_box_box_on_paper():
  # unit-free: A half (.1, .1) at the origin; B half (.1, .1)
  # B turned by 45 degrees, its corner (-.1 sqrt 2 from its centre) .02 inside A's +x face: one vertex of B only
  bx = 0.1 - 0.02 + 0.1 * math.sqrt(2)
  _hit(cr.box_box(0, 0, 0, 0.1, 0.1, bx, 0, math.pi / 4, 0.1, 0.1), 'bb', 0.02, (0, 1))
  _hit(cr.box_box(bx, 0, math.pi / 4, 0.1, 0.1, 0, 0, 0, 0.1, 0.1), 'bb', 0.02, (1, 0))
  # two aligned boxes offset by (.15, .15): one vertex of each in the other, .05 from both faces
  _hit(cr.box_box(0, 0, 0, 0.1, 0.1, 0.15, 0.15, 0, 0.1, 0.1), 'bb', 0.05, (1, 1))
  # a small box (.02) poking .01 through A's +x face: two of its vertices inside, none of A's in it
  _hit(cr.box_box(0, 0, 0, 0.1, 0.1, 0.11, 0, 0, 0.02, 0.02), 'bb', 0.01, (0, 2))
  # a plus sign: the boxes overlap, no vertex of either inside the other - no contact in the specification
  _hit(cr.box_box(0, 0, 0, 0.3, 0.05, 0, 0, math.pi / 2, 0.3, 0.05), 'bb', 0.0, (0, 0))
  assert cr.box_box(0, 0, 0, 0.1, 0.1, 0.2, 0, 0, 0.1, 0.1) is None        # faces touching
  assert cr.box_box(0, 0, 0, 0.1, 0.1, 0.25, 0, math.pi / 4, 0.1, 0.1) is None   # the corner .0086 short of the face
  # the vertex criterion is strict: a vertex ON the face is not inside
  assert cr.box_box(0, 0, 0, 0.1, 0.1, 0.1 + 0.1 * math.sqrt(2), 0, math.pi / 4, 0.1, 0.1) is None


def _record(robot_pose=(0, 0, 0), task=3, vases=(), pillars=(), buttons=(), obj=None, awake=0):
  rf, ri = np.zeros(REC_FLOATS, np.float32), np.zeros(REC_INTS, np.int32)
  rf[F_ROBOT:F_ROBOT + 3] = robot_pose
  rf[F_VASE_SIZE], rf[F_PILLAR_SIZE] = 0.1, 0.2
  ri[I_TASK], ri[I_NV], ri[I_NP], ri[I_NB], ri[I_AWAKE] = task, len(vases), len(pillars), len(buttons), awake
  for k, v in enumerate(vases):
    rf[F_VASES + 6 * k:F_VASES + 6 * k + len(v)] = v
  for k, p in enumerate(pillars):
    rf[F_PILLARS + 2 * k:F_PILLARS + 2 * k + 2] = p
  for k, b in enumerate(buttons):
    rf[F_BUTTONS + 2 * k:F_BUTTONS + 2 * k + 2] = b
  if obj:
    ri[I_BOX_KIND] = obj[0]
    rf[F_BOX:F_BOX + len(obj[1])] = obj[1]
  return rf, ri


def _keys(cen):
  return {o.key: o for o in cen.overlaps}


def test_census_point_footprint_and_pair_order():
  # Point at the origin facing +y: the sphere r .1 at the origin, the arrow box (.05) centred at (0, .1)
  rf, ri = _record(robot_pose=(0, 0, math.pi / 2), pillars=[(0.0, 0.33)], buttons=[(0.17, 0.0)],
                   vases=[(-0.18, 0.0, 0.0, 0.1, 0, 0), (5.0, 5.0, 0.0), (-0.35, 0.05, 0.0)])
  cen = cr.census(rf, ri, 'point')
  k = _keys(cen)
  assert set(k) == {('robot', 'pillar', 1, 0, 'cb-face'), ('robot', 'button', 0, 0, 'cc'), ('robot', 'vase', 0, 0, 'cb-face'),
                    ('vase', 'vase', 0, 0, 'bb')}
  assert k['robot', 'pillar', 1, 0, 'cb-face'].depth == pytest.approx(0.02, abs=1e-7)   # the arrow's far face at y = .15, the pillar from .13
  assert k['robot', 'button', 0, 0, 'cc'].depth == pytest.approx(0.03, abs=1e-7)
  assert k['robot', 'vase', 0, 0, 'cb-face'].depth == pytest.approx(0.02, abs=1e-7)
  vv = k['vase', 'vase', 0, 0, 'bb']
  # (aligned boxes offset by .05 in y: one vertex each, .03 from the x face)
  assert (vv.ia, vv.ib, vv.verts) == (0, 2, (1, 1)) and vv.depth == pytest.approx(0.03, abs=1e-7)
  assert cen.n_dynamic == 1 and cen.taut is None
  # vase 0 moves, vase 2 sleeps and the robot does not touch it, but nothing else lies on vase 2: no chain
  assert cr.wake_chains(rf, ri, 'point', cen.overlaps) == []
  ri[I_AWAKE] = 0b101
  assert cr.census(rf, ri, 'point').n_dynamic == 2
  # one more sleeper on vase 2 (its vertex (-.45, .15) .05 inside vase 1) makes one
  rf, ri = _record(robot_pose=(0, 0, math.pi / 2), vases=[(-0.18, 0.0, 0.0, 0.1, 0, 0), (-0.5, 0.1, 0.0), (-0.35, 0.05, 0.0)])
  cen = cr.census(rf, ri, 'point')
  assert cr.wake_chains(rf, ri, 'point', cen.overlaps) == [(0, 2, 1)]
  ri[I_AWAKE] = 0b010   # the far sleeper flagged awake: the pair walk evaluates its pair anyway
  assert cr.wake_chains(rf, ri, 'point', cen.overlaps) == []


def test_census_ball_presents_its_reduced_radius_to_the_sphere_only():
  # the sphere touches the ball at sqrt(.24^2 - .04^2) = .23664; the arrow (front face at x = .15) meets its full .14
  assert cr.BALL_TO_SPHERE == pytest.approx(0.13664319, abs=1e-8)
  for d, sphere, arrow in ((0.238, False, True), (0.236, True, True), (0.285, False, True), (0.295, False, False)):
    rf, ri = _record(task=2, obj=(cr.BOX_BALL, (d, 0.0, 0.0)))
    k = _keys(cr.census(rf, ri, 'point'))
    assert (('robot', 'object', 0, 0, 'cc') in k) == sphere, d
    assert (('robot', 'object', 1, 0, 'cb-face') in k) == arrow, d
  assert k == {}
  rf, ri = _record(task=2, obj=(cr.BOX_BALL, (0.2, 0.0, 0.0)))
  k = _keys(cr.census(rf, ri, 'point'))
  assert k['robot', 'object', 0, 0, 'cc'].depth == pytest.approx(0.1 + cr.BALL_TO_SPHERE - 0.2, abs=1e-7)
  assert k['robot', 'object', 1, 0, 'cb-face'].depth == pytest.approx(0.14 - 0.05, abs=1e-7)   # the ball's centre .05 in front of the arrow


def test_census_box_rod_car_and_tether():
  # the five geoms of the PushBox box: a vase tucked against the main box's +x face between the corner columns at y = +-.2
  rf, ri = _record(robot_pose=(5, 5, 0), task=10, vases=[(0.29, 0.02, 0.0)], obj=(cr.BOX_BOX, (0.0, 0.0, 0.0)))
  k = _keys(cr.census(rf, ri, 'point'))
  assert set(k) == {('vase', 'object', 0, 0, 'bb'), ('vase', 'object', 0, 1, 'bb')}   # (the column at (.2, -.2) ends at y = -.1, the vase at -.08)
  assert k['vase', 'object', 0, 0, 'bb'].verts == (2, 0) and k['vase', 'object', 0, 0, 'bb'].depth == pytest.approx(0.01, abs=1e-7)
  assert k['vase', 'object', 0, 1, 'bb'].verts == (1, 1) and k['vase', 'object', 0, 1, 'bb'].depth == pytest.approx(0.02, abs=1e-7)
  # the rod (.08 x .3 along its y) turned by 90 degrees lies along x
  rf, ri = _record(robot_pose=(0, 0.16, 0), task=12, obj=(cr.BOX_ROD, (0.0, 0.0, math.pi / 2)))
  k = _keys(cr.census(rf, ri, 'point'))
  assert k['robot', 'object', 0, 0, 'cb-face'].depth == pytest.approx(0.02, abs=1e-7)
  assert set(k) == {('robot', 'object', 0, 0, 'cb-face')}   # (the arrow's lower face at y = .11, the rod's upper at .08)
  # Car at the origin, yaw 0: its rear ball (geom 7, r .05) at (0, -.1), front bumper (geom 3) down to y = -.175, wheels (5, 6) at x = -+.13
  rf, ri = _record(task=10, pillars=[(0.0, -0.34)], vases=[(0.24, 0.1, 0.0)])
  k = _keys(cr.census(rf, ri, 'car'))
  assert set(k) == {('robot', 'pillar', 3, 0, 'cb-face'), ('robot', 'pillar', 4, 0, 'cb-face'), ('robot', 'pillar', 7, 0, 'cc'),
                    ('robot', 'vase', 6, 0, 'bb')}
  assert k['robot', 'pillar', 3, 0, 'cb-face'].depth == pytest.approx(0.035, abs=1e-7)   # the bumper down to y = -.175, the pillar up to -.14
  assert k['robot', 'pillar', 4, 0, 'cb-face'].depth == pytest.approx(0.02, abs=1e-7)    # the connector down to -.16
  assert k['robot', 'pillar', 7, 0, 'cc'].depth == pytest.approx(0.01, abs=1e-7)         # the centres .24 apart
  assert k['robot', 'vase', 6, 0, 'bb'].verts == (2, 0) and k['robot', 'vase', 6, 0, 'bb'].depth == pytest.approx(0.015, abs=1e-7)
  # the tether: L = sqrt(d^2 + .1^2) against .75, i.e. d against sqrt(.75^2 - .01) = .74330
  for d, taut in ((0.74, False), (0.745, True)):
    rf, ri = _record(task=cr.TASK_HAUL_BOX, obj=(cr.BOX_BOX, (d, 0.0, 0.0)))
    assert cr.census(rf, ri, 'point').taut is taut


@pytest.mark.parametrize('name', list(cr.CASES))
def test_installed_states_reach_the_case_table(name):
  robot, task = cr.CASES[name][:2]
  n = 192
  rf, ri, awake = cr.directed_records(name, n, bu.sample_records_native(robot, task, n, seed=cr.CASE_SEED[name]))
  ri[:, I_AWAKE] = awake
  tally = cr.Tally()
  cen = [cr.census(rf[e], ri[e], robot) for e in range(n)]
  for c in cen:
    tally.add(c.overlaps)
  missed = [r for r in cr.reach(name, tally) if r[1] < r[3]]
  assert not missed, missed
  if name == 'vase_crowd':
    assert min(c.n_dynamic for c in cen) >= 4
  if name == 'wake_order':
    assert sum(bool(cr.wake_chains(rf[e], ri[e], robot, cen[e].overlaps)) for e in range(n)) >= 20
  if task == 'haul_box':
    assert sum(c.taut is True for c in cen) >= 20 and sum(c.taut is False for c in cen) >= 20

"""The ray caster k_render_rgb (csrc/sag_render.hpp: r_render_env<R_OUT_RGB>, the colour branch of its pixel loop) and the oracle's twin
of it (oracle/sag_oracle_render.inc) against the independent per-pixel reference tests/render_ref.py.  One list of cases, used three times:
  (a) reference vs oracle, no GPU: judges the oracle;
  (b) device vs reference through the C ABI (sag_render_device into a caller's buffer at a byte offset of 3);
  (c) the cases of (b) on the ASan / UBSan host build of the library's sources.
Every comparison makes the same assertion, render_ref.check(): decided pixels equal in every channel, an edge-undecided
pixel equal to one of its five evaluations to +-1 level, at most 1 edge-undecided pixel in 10 000 (render_ref's docstring
has the rule in full, with the two surfaces of one place - a Doggo's knee spheres - that may show either colour).  What a case is FOR
(more than 12 layers, a flat cap in view, a bounding-sphere centre behind the ray, ...) is asserted from the reference."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import render_ref as rr
from oracle_lib import (F_BOX, F_BUTTONS, F_GOAL, F_HAZARD_SIZE, F_HAZARDS, F_PILLARS, F_ROBOT, F_ROBOT_EXT, F_VASES, I_ACTIVE_MASK,
                        I_BTN_STATE, Oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RID = {'point': 0, 'car': 1, 'doggo': 2}
CAM = {'vision': 0, 'fixednear': 1, 'fixedfar': 2, 'track': 3}
FAR = (2.9, 2.9)   # where a body goes that a case does not need
JOINT_RANGE_DEG = np.array([(-10, 30), (-75, 15), (-75, 0), (-10, 30), (-75, 15), (-75, 0), (-30, 30), (-10, 30), (0, 135), (-75, 0),
                            (-10, 30), (0, 135), (-75, 0)], np.float64)   # doggo.xml:21-71 in qpos order
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def oracle():
  return Oracle()


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
def _record(robot, task, nh=0, nv=0, np_=0, nb=0, xy=(0.0, 0.0), yaw=0.0, goal=FAR):
  names = (['robot', 'goal'] + [f'hazards{k}' for k in range(nh)] + [f'vases{k}' for k in range(nv)] +
           [f'pillars{k}' for k in range(np_)] + [f'buttons{k}' for k in range(nb)])
  rf, ri = gu.base_record(task, names, {'robot': 0.4}, robot=robot)
  rf[F_ROBOT:F_ROBOT + 3] = [xy[0], xy[1], yaw]
  rf[F_GOAL:F_GOAL + 2] = goal
  rf[F_BOX:F_BOX + 2] = (-2.9, 2.9)
  for base, cnt, stride in ((F_HAZARDS, nh, 2), (F_VASES, nv, 6), (F_PILLARS, np_, 2), (F_BUTTONS, nb, 2)):
    for k in range(cnt):
      rf[base + stride * k:base + stride * k + 2] = (-2.9 + 0.3 * k, -2.9)
  if robot == 'doggo':
    _doggo_pose(rf, 0.22, [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
  return rf, ri


def _doggo_pose(rf, z, quat, joints=None):
  E = F_ROBOT_EXT
  rf[E:E + 40] = 0
  rf[E] = z
  rf[E + 1:E + 5] = np.asarray(quat, np.float64) / np.linalg.norm(quat)
  if joints is not None:
    rf[E + 9:E + 22] = joints


def _stack(recs):
  return np.stack([r[0] for r in recs]).astype(np.float32), np.stack([r[1] for r in recs]).astype(np.int32)


def _sampled(robot, task, n, seed):
  import batch_util as bu
  rf, ri = bu.sample_records_native(robot, task, n, seed=seed)
  rf = rf.astype(np.float32)
  if robot == 'doggo':   # (a zero quaternion means "upright at ROBOT yaw": written out, so that every reader sees one pose)
    for k in range(n):
      if not rf[k, F_ROBOT_EXT + 1:F_ROBOT_EXT + 5].any():
        _doggo_pose(rf[k], 0.22, [np.cos(rf[k, 2] / 2), 0, 0, np.sin(rf[k, 2] / 2)])
  return rf, ri


# ---------------------------------------------------------------------------------------------------------------------
# what a case is for, asserted from the reference images
# ---------------------------------------------------------------------------------------------------------------------
def _px(refs, f):
  return int(sum(f(r).sum() for r in refs))


def _surface(r, prefix, part=None):
  idx = [k for k, g in enumerate(r.geoms) if g.name.startswith(prefix)]
  m = np.isin(r.surf, idx)
  return m if part is None else m & (r.part == part)


def _expect_layers(refs):
  n = _px(refs, lambda r: r.layers > rr.MAX_LAYERS)
  assert n >= 30, f'{n} pixels with more than {rr.MAX_LAYERS} translucent entries: fix the placement'
  assert all(r.geoms[-1].name == 'cost' for r in refs), 'the cost sphere (last geom, nearest layer) must be drawn'


def _expect_caps(prefixes):
  def f(refs):
    for p in prefixes:
      for part in (1, 2):
        n = _px(refs, lambda r: _surface(r, p, part))
        assert n >= 20, f'cap {part} of {p} is seen in {n} pixels'
  return f


def _expect_outer_caps(refs):
  """The Doggo's torso cylinders meet at the waist: their caps there face each other and no ray reaches them.  The nose
  (front cylinder, end e) and the tail (rear cylinder, end a) are the caps in view."""
  for name, part in (('doggo0', 2), ('doggo7', 1)):
    n = _px(refs, lambda r: _surface(r, name, part))
    assert n >= 20, f'cap {part} of {name} is seen in {n} pixels'


def _expect_behind(refs):
  assert _px(refs, lambda r: r.behind) > 0, 'no visible geom has its bounding-sphere centre behind the ray'


def _expect_inside(names):
  def f(refs):
    for r in refs:
      assert [g.name for g in r.geoms if g.name in names] == list(names)
      o = r.origin
      for g in r.geoms:
        if g.name in names:
          t = g.hit(o, np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.6, 0.0, -0.8]]))[0]
          assert not np.isfinite(t).any(), f'the camera is not inside {g.name}'
  return f


def _expect_seen(*prefixes):
  """The opaque geoms are in view, some of their pixels under a translucent layer."""
  def f(refs):
    for p in prefixes:
      assert _px(refs, lambda r: _surface(r, p)) >= 10, f'{p} is not in view'
      assert _px(refs, lambda r: _surface(r, p) & (r.layers > 0)) > 0, f'no layer in front of {p}'
  return f


def _expect_seen_opaque(*names):
  def f(refs):
    for p in names:
      if p == 'box':   # translucent: a layer, not a surface
        assert any(g.name == 'box' for g in refs[0].geoms) and _px(refs, lambda r: r.layers > 0) >= 10
      else:
        assert _px(refs, lambda r: _surface(r, p)) >= 10, f'{p} is not in view'
  return f


# ---------------------------------------------------------------------------------------------------------------------
# the cases: name -> (robot, camera, W, H, overlays, records(), expectation or None)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(name, robot, camera, W, H, overlays, records, expect=None):
  assert name not in CASES
  CASES[name] = (robot, camera, W, H, overlays, records, expect)


# image sizes: multiples of the 8 x 8 tile and not, fewer pixels than a wavefront, than the block, wider than tall
for _W, _H in ((64, 64), (1, 1), (7, 5), (8, 8), (9, 8), (50, 37), (130, 50)):
  for _n in (1, 3):
    _case(f'size {_W}x{_H} N={_n}', 'point', 'track', _W, _H, True, lambda n=_n: _sampled('point', 'push_box', n, seed=40 + n))


def _layers_records():
  recs = []
  for yaw in (0.0, 2.0, -1.2):
    # (the goal more than its .3 from the box: a box in the goal would end the episode's stage and move the goal)
    rf, ri = _record('point', 'push_box', nh=9, yaw=yaw, goal=(-0.2, 0.0))
    rf[F_HAZARD_SIZE] = 0.6
    rf[F_HAZARDS:F_HAZARDS + 18] = np.tile([0.05, 0.0], 9)
    rf[F_BOX:F_BOX + 3] = [0.15, 0.1, 0.6]
    recs.append((rf, ri))
  return _stack(recs)


for _cam in ('fixednear', 'track'):
  _case(f'more than 12 layers, {_cam}', 'point', _cam, 96, 64, True, _layers_records, _expect_layers)


def _car_yaw_records(camera):
  recs = []
  if camera == 'track':   # the tracking camera sees a wheel's flat end only of a car turned towards it: four more yaws
    for yaw in (0.0, np.pi / 2, np.pi, -np.pi / 2, 0.9, -0.9, 2.2, -2.2):
      recs.append(_record('car', 'go_to_goal', yaw=yaw))
  else:   # fixednear looks along +y from (0, -2, 2): the cars stand to its left and right, so that it sees the flat ends from
    #       both sides - the inner ones through the gap between body and bumper (car.xml:16-17,23,27)
    for xy, yaw in (((-0.8, -0.6), 0.0), ((0.5, -0.9), np.pi / 2), ((0.8, -0.5), np.pi), ((-0.5, -0.9), -np.pi / 2),
                    ((0.7, -1.0), np.pi / 2), ((-0.7, -1.0), -np.pi / 2)):
      recs.append(_record('car', 'go_to_goal', xy=xy, yaw=yaw))
  return _stack(recs)


_case('car wheel caps, track', 'car', 'track', 192, 128, False, lambda: _car_yaw_records('track'))
_case('car wheel caps, fixednear', 'car', 'fixednear', 320, 240, False, lambda: _car_yaw_records('fixednear'))


def _qz(a):
  return np.array([np.cos(a / 2), 0, 0, np.sin(a / 2)])


def _qx(a):
  return np.array([np.cos(a / 2), np.sin(a / 2), 0, 0])


def _qmul(a, b):
  return np.r_[a[0] * b[0] - a[1:] @ b[1:], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])]


def _doggo_tipped_records():
  rng = np.random.RandomState(7)
  # upside down about x and about y, four random, two with the tail towards fixednear (yaw 90 degrees, then rolled)
  quats = [(0, 1, 0, 0), (0, 0, 1, 0)] + [rng.randn(4) for _ in range(4)] + [_qmul(_qz(np.pi / 2), _qx(a)) for a in (1.0, -2.4)]
  recs = []
  for k, q in enumerate(quats):
    rf, ri = _record('doggo', 'go_to_goal', xy=(0.4 * (k % 3) - 0.4, -0.6 + 0.5 * (k // 3)))
    ends = np.radians(JOINT_RANGE_DEG[np.arange(13), rng.randint(0, 2, 13)])
    _doggo_pose(rf, 0.6, q, ends)
    recs.append((rf, ri))
  return _stack(recs)


for _cam in ('fixednear', 'vision'):
  _case(f'doggo tipped, joints at their range ends, {_cam}', 'doggo', _cam, 128, 96, False, _doggo_tipped_records, None)


def _touching_records(robot):
  """The robot against a PushBox box (bounding sphere .35) and a vase (.17): the camera is inside both spheres at some yaws
  and turned away from their centres at others."""
  recs = []
  for yaw in (0.0, 0.7, 1.3, 1.9, 2.5, -2.2):
    rf, ri = _record(robot, 'push_box', nv=1, yaw=yaw)
    rf[F_BOX:F_BOX + 3] = [0.31 if robot == 'point' else 0.36, 0.0, 0.0]   # its face 1 cm from the Point's sphere / 5 mm from the Car's wheel
    rf[F_VASES:F_VASES + 3] = [0.0, 0.21, 0.3]
    recs.append((rf, ri))
  return _stack(recs)


for _robot in ('point', 'car'):
  _case(f'camera inside a bounding sphere: {_robot} touching a box and a vase', _robot, 'vision', 64, 64, False,
        lambda r=_robot: _touching_records(r), _expect_seen_opaque('box', 'vase'))


def _inside_records():
  recs = []
  for yaw in (0.0, 1.0, -2.4, -1.5):
    rf, ri = _record('point', 'push_box', nh=1, yaw=yaw, goal=(0.05, -0.03))   # (push_box: standing in the goal ends nothing)
    # the hazard's centre .35 m behind a robot that looks along -2.4 rad, its disc .45 m out in front: seen from .25 m above,
    # centre and hit point are more than a right angle apart (.35 x .45 > .25^2)
    rf[F_HAZARDS:F_HAZARDS + 2] = [0.25, 0.25]
    rf[F_HAZARD_SIZE] = 0.8
    recs.append((rf, ri))
  return _stack(recs)


# (the hazard under the robot reaches out in front of the camera while its centre lies behind it)
_case('camera inside a bounding sphere: the goal cylinder and the cost sphere', 'point', 'vision', 64, 64, True, _inside_records, _expect_inside(('goal', 'cost')))


def _surface_records(kind):
  recs = []
  for yaw in (0.3, 2.0, -2.4):
    if kind == 'rod':   # a hazard disc under a vase and under the rod
      rf, ri = _record('point', 'roll_rod', nh=2, nv=1, xy=(0.0, -0.9), yaw=yaw)
      rf[F_HAZARDS:F_HAZARDS + 4] = [0.5, 0.1, -0.5, 0.1]
      rf[F_VASES:F_VASES + 3] = [0.5, 0.15, 0.4]
      rf[F_BOX:F_BOX + 3] = [-0.5, 0.05, 1.0]
    else:               # the box's columns against a pillar, the goal intersecting another
      rf, ri = _record('point', 'push_box', np_=2, xy=(0.0, -0.9), yaw=yaw, goal=(-0.6, 0.2))
      rf[F_PILLARS:F_PILLARS + 4] = [0.5 + 0.3 + 0.2, 0.2, -0.8, 0.3]
      rf[F_BOX:F_BOX + 3] = [0.5, 0.0, 0.0]
    recs.append((rf, ri))
  return _stack(recs)


for _kind in ('rod', 'columns'):
  for _cam in ('fixednear', 'track'):
    _case(f'layers at the opaque surface, {_kind}, {_cam}', 'point', _cam, 96, 64, False, lambda k=_kind: _surface_records(k))


def _edge_records(robot):
  """At (3.4, 3.4), 10 cm from both edges of the floor, looking outward (all sky beyond the robot's own nose) and inward; further
  in, looking out over the corner and over one edge, where the floor's last squares and the sky share the image."""
  turn = np.pi / 2 if robot == 'car' else 0.0   # the Car's camera looks along -y of its body (car.xml:14) ...
  d = 0.25 if robot == 'car' else 0.1           # ... and with its 45 degrees sees the floor from .31 m on, the Point from .11 m
  return _stack([_record(robot, 'go_to_goal', xy=xy, yaw=phi + turn, goal=(2.0, 2.0)) for xy, phi in (
      ((3.4, 3.4), np.pi / 4), ((3.4, 3.4), -3 * np.pi / 4), ((3.5 - 3 * d, 3.5 - 3 * d), np.pi / 4), ((3.5 - 4 * d, 3.4), 0.0),
      ((3.4, 3.5 - 6 * d), np.pi / 2))])


def _expect_sky_and_floor(refs):
  assert (refs[0].surf == -1).sum() < 50 < (refs[0].surf == -2).sum(), 'looking outward from the corner: sky, no floor to speak of'
  for r in refs[1:]:
    assert (r.surf == -2).sum() >= 50 and (r.surf == -1).sum() >= 50, 'sky and floor must both be in view'


_case('floor edge and sky, point', 'point', 'vision', 64, 64, False, lambda: _edge_records('point'), _expect_sky_and_floor)
_case('floor edge and sky, car', 'car', 'vision', 64, 64, False, lambda: _edge_records('car'), _expect_sky_and_floor)
_case('floor edge and sky, fixedfar', 'point', 'fixedfar', 96, 64, True, lambda: _edge_records('point'))


def _buttons_records():
  rf, ri = _sampled('point', 'press_buttons', 4, seed=51)
  ri[:2, I_BTN_STATE] = 0        # BUTTON_CHANGE: every button pink (press_buttons.py:82); NORMAL: the goal button green
  ri[2:, I_BTN_STATE] = 1
  return rf, ri


def _collect_records():
  rf, ri = _sampled('car', 'collect', 3, seed=52)
  ri[:, I_ACTIVE_MASK] = [0b101010, 0b000111, 0b111111]
  return rf, ri


_case('unsupervised', 'point', 'fixednear', 96, 64, True, lambda: _sampled('point', 'unsupervised', 4, seed=53))
_case('box kind box', 'car', 'track', 96, 64, True, lambda: _sampled('car', 'push_box', 3, seed=54))
_case('box kind rod', 'point', 'track', 96, 64, True, lambda: _sampled('point', 'roll_rod', 3, seed=55))
_case('box kind ball', 'point', 'track', 96, 64, True, lambda: _sampled('point', 'dribble_ball', 3, seed=56))
_case('press_buttons in both button states', 'point', 'fixednear', 96, 64, True, _buttons_records)
_case('collect with three active masks', 'car', 'fixedfar', 96, 64, True, _collect_records)


def _fullest_records():
  rng = np.random.RandomState(3)
  recs = []
  for k in range(3):
    rf, ri = _record('doggo', 'push_box', nh=9, nv=10, np_=2, nb=6, xy=rng.uniform(-0.5, 0.5, 2), yaw=rng.uniform(-3, 3),
                     goal=rng.uniform(-1.5, 1.5, 2))
    for base, cnt, stride in ((F_HAZARDS, 9, 2), (F_VASES, 10, 6), (F_PILLARS, 2, 2), (F_BUTTONS, 6, 2)):
      for j in range(cnt):
        rf[base + stride * j:base + stride * j + 2] = rng.uniform(-2, 2, 2)
        if stride == 6:
          rf[base + stride * j + 2] = rng.uniform(-3, 3)
    rf[F_BOX:F_BOX + 3] = [*rng.uniform(-1.5, 1.5, 2), rng.uniform(-3, 3)]
    rf[F_HAZARDS:F_HAZARDS + 2] = rf[F_ROBOT:F_ROBOT + 2]   # the cost flag up: the cost sphere is drawn
    recs.append((rf, ri))
  return _stack(recs)


def _expect_fullest(refs):
  for r in refs:
    assert len(r.geoms) == 96 <= rr.MAX_GEOMS   # 9 + 10 + 2 + goal + 6 + box and columns + 14 + 48 rings + cost


_case('fullest scene', 'doggo', 'fixedfar', 96, 64, True, _fullest_records, None)

# the robot / task (/ camera) pairs of test_gpu_parity.test_rgb_observation_matches_oracle and test_human_view_matches_oracle
for _robot, _task in (('point', 'go_to_goal'), ('point', 'press_buttons'), ('point', 'push_box'), ('car', 'dribble_ball'), ('car', 'collect'),
                      ('doggo', 'go_to_goal'), ('doggo', 'roll_rod'), ('point', 'unsupervised'), ('doggo', 'haul_box')):
  _case(f'rgb {_robot} {_task}', _robot, 'vision', 64, 64, False, lambda r=_robot, t=_task: _sampled(r, t, 8, seed=31))
for _robot, _task, _cam in (('point', 'go_to_goal', 'fixedfar'), ('car', 'push_box', 'track'), ('doggo', 'press_buttons', 'fixednear'),
                            ('point', 'collect', 'vision')):
  _case(f'human view {_robot} {_task} {_cam}', _robot, _cam, 96, 64, True, lambda r=_robot, t=_task: _sampled(r, t, 8, seed=77))

# expectations that hold over a group of cases (a flat end faces one camera or the other, not both)
GROUPS = {
    'camera inside a bounding sphere': _expect_behind,
    'car wheel caps': _expect_caps(('wheel0', 'wheel1')),
    'doggo tipped': _expect_outer_caps,
    'layers at the opaque surface, rod': _expect_seen('vase', 'rod'),
    'layers at the opaque surface, columns': _expect_seen('pillar'),
    'fullest scene': _expect_fullest,
}


# ---------------------------------------------------------------------------------------------------------------------
# reference images, computed once per (records, overlay inputs)
# ---------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _references(oracle, robot, camera, W, H, overlays, rf, ri, obs, cost):
  rid, cam = RID[robot], CAM[camera]
  key = (rid, cam, W, H, overlays, rf.tobytes(), ri.tobytes(), obs[:, :48].tobytes() if overlays else b'', cost.tobytes() if overlays else b'')
  if key not in _REFS:
    _REFS[key] = rr.render_batch(oracle, rf, ri, rid, cam, W, H, overlays, obs, cost)
  return _REFS[key]


def _oracle_overlay_inputs(oracle, robot, rf, ri):
  """Observation and cost flag of the records as they stand (a step of no substeps)."""
  outs = [oracle.step(oracle.env(rf[k], ri[k]), RID[robot], np.zeros(12), noise=np.zeros(12), nstep=0) for k in range(len(rf))]
  return np.array([o.obs[:48] for o in outs], np.float32), np.array([o.cost for o in outs], np.uint8)


def _oracle_case(oracle, name):
  robot, camera, W, H, overlays, records, expect = CASES[name]
  rf, ri = records()
  assert 1 <= len(rf) <= 8
  obs, cost = _oracle_overlay_inputs(oracle, robot, rf, ri)
  return _references(oracle, robot, camera, W, H, overlays, rf, ri, obs, cost), (rf, ri, obs, cost)


# ---------------------------------------------------------------------------------------------------------------------
# (a) reference vs oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_oracle_image_equals_the_reference(oracle, name):
  robot, camera, W, H, overlays, records, expect = CASES[name]
  refs, (rf, ri, obs, cost) = _oracle_case(oracle, name)
  if expect:
    expect(refs)
  img = np.stack([oracle.render(oracle.env(rf[k], ri[k]), RID[robot], CAM[camera], W, H, overlays, obs[k], cost[k]) for k in range(len(rf))])
  total, und, alt = rr.check(img, refs, name)
  print(f'{name}: {total} pixels, {und} edge-undecided, {alt} on coincident surfaces show the later geom')


@pytest.mark.parametrize('group', list(GROUPS))
def test_cases_show_what_they_are_for(oracle, group):
  names = [n for n in CASES if n.startswith(group)]
  assert names
  GROUPS[group]([r for n in names for r in _oracle_case(oracle, n)[0]])


def test_reference_known_answers():
  """The reference's own primitives against hand-computed rays: entry points, normals, faces, and nothing from inside."""
  o = np.zeros(3)
  d = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
  t, n, part = rr.Sphere('s', (3, 0, 0), 1.0, (1, 1, 1), 1.0).hit(o, d)
  assert t[0] == 2.0 and np.isinf(t[1:]).all() and (n[0] == [-1, 0, 0]).all()
  assert np.isinf(rr.Sphere('s', (0.2, 0, 0), 1.0, (1, 1, 1), 1.0).hit(o, d)[0]).all()        # the camera inside
  t, n, part = rr.Box('b', (3, 0, 0), (1, 2, 3), 0.0, (1, 1, 1), 1.0).hit(o, d)
  assert t[0] == 2.0 and (n[0] == [-1, 0, 0]).all() and part[0] == 1 and np.isinf(t[1])
  np.testing.assert_allclose(t[2], 2.0 / 0.6, rtol=1e-15)                                      # (x = 2 at z = 2.67 < 3)
  t, n, part = rr.Box('b', (3, 0, 0), (1, 1, 1), np.pi / 4, (1, 1, 1), 1.0).hit(o, d)
  np.testing.assert_allclose(t[0], 3 - np.sqrt(2), rtol=1e-15)                                 # the corner of the turned box
  cyl = rr.Rod('c', (2, 0, -1), (4, 0, -1), 0.5, False, (1, 1, 1), 1.0)                        # along x, below the origin
  t, n, part = cyl.hit(o, np.array([[0.0, 0.0, -1.0], [0.6, 0.0, -0.2], [3.0, 0.0, -0.5]]) / [[1.0], [np.sqrt(0.4)], [np.sqrt(9.25)]])
  assert np.isinf(t[0]) and part[1] == 1 and (n[1] == [-1, 0, 0]).all() and part[2] == 0      # miss, the cap at a, the side
  np.testing.assert_allclose(t[1] * 0.6 / np.sqrt(0.4), 2.0, rtol=1e-15)
  cap = rr.Rod('c', (2, 0, 0), (4, 0, 0), 0.5, True, (1, 1, 1), 1.0)
  t, n, part = cap.hit(o, d)
  assert t[0] == 1.5 and part[0] == 1 and (n[0] == [-1, 0, 0]).all()                          # the end sphere at a
  t, n, part = cap.hit(np.array([10.0, 0, 0]), -d)
  assert t[0] == 5.5 and part[0] == 2 and (n[0] == [1, 0, 0]).all()                           # the end sphere at e
  # compositing: nine coincident discs (alpha .25, lit fully from above) over the floor
  rf, ri = _record('point', 'go_to_goal', nh=9, xy=FAR)
  rf[F_HAZARDS:F_HAZARDS + 18] = 0.0
  rf[F_HAZARD_SIZE] = 0.9
  im = rr.render(rf.astype(np.float32), ri, 0, CAM['fixedfar'], 8, 8, False)
  m = (im.layers == 9) & (im.surf == -1)
  assert m.sum() >= 2
  grey = np.where(im.part[m] == 1, 0.8, 0.7)
  np.testing.assert_allclose(im.colour[0][m], np.stack([grey * 0.75**9, grey * 0.75**9, 1 - (1 - grey) * 0.75**9], -1), rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------
# (b) device vs reference through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _device_images(nat, ctx, cam, W, H, overlays, obs, cost):
  """sag_render_device into a caller's buffer at a byte offset of 3, sentinel bytes before and after."""
  n = ctx.n_envs
  size, tail = n * H * W * 3, 5
  d_out = ctx.dev_alloc(3 + size + tail)
  ctx.dev_upload(d_out, np.full(3 + size + tail, SENTINEL, np.uint8))
  d_obs = d_cost = None
  if overlays:
    d_obs, d_cost = ctx.dev_alloc(obs.nbytes), ctx.dev_alloc(n)
    ctx.dev_upload(d_obs, np.ascontiguousarray(obs, np.float32))
    ctx.dev_upload(d_cost, np.ascontiguousarray(cost, np.uint8))
  ctx._check(ctx.lib.sag_render_device(ctx.h, cam, W, H, 1 if overlays else 0, d_obs, d_cost, C.c_void_p(d_out.value + 3)),
             'sag_render_device')
  ctx.wait()
  buf = ctx.dev_download(d_out, (3 + size + tail,), np.uint8)
  for p in (d_out, d_obs, d_cost):
    if p is not None:
      ctx.dev_free(p)
  assert (buf[:3] == SENTINEL).all() and (buf[3 + size:] == SENTINEL).all(), 'bytes outside the image were written'
  return buf[3:3 + size].reshape(n, H, W, 3)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_device_image_equals_the_reference(nat, oracle, name):
  robot, camera, W, H, overlays, records, expect = CASES[name]
  rf, ri = records()
  n = len(rf)
  ctx = nat.Context(robot, n, seed=5)
  ctx.set_layout(rf, ri)
  out = ctx.step(np.zeros((n, ctx.info['nu']), np.float32), nstep=0)
  obs, cost = out[0], out[2]
  rf2, ri2 = ctx.get_state()
  same = np.r_[0:2, 24:27, 32:34, 41:44, 47:141, 144:149, 153:166]   # poses and sizes: the step of no substeps moved nothing
  np.testing.assert_array_equal(rf2[:, same], rf[:, same], err_msg='the scene is no longer the case')
  scene_ints = np.r_[0:8, 10]   # task, counts, box kind, goal button, button state, active mask
  np.testing.assert_array_equal(ri2[:, scene_ints], ri[:, scene_ints], err_msg='the scene is no longer the case')
  img = _device_images(nat, ctx, CAM[camera], W, H, overlays, obs, cost)
  ctx.close()
  refs = _references(oracle, robot, camera, W, H, overlays, rf2, ri2, obs, cost)
  if expect:
    expect(refs)
  total, und, alt = rr.check(img, refs, name)
  print(f'{name}: {total} pixels, {und} edge-undecided, {alt} on coincident surfaces show the later geom')
  assert W * H < 64 or len(np.unique(img.reshape(-1, 3), axis=0)) > 3, 'a flat image'


# ---------------------------------------------------------------------------------------------------------------------
# (c) the cases of (b) on the sanitizer host build
# ---------------------------------------------------------------------------------------------------------------------
def test_render_cases_on_the_sanitizer_build():
  """This file's GPU cases on the ASan / UBSan host build of the library's sources (tests/hostemu), as
  test_async_reset.test_async_reset_cases_on_the_sanitizer_build: no report, every case passed, none skipped."""
  sys.path.insert(0, os.path.join(ROOT, 'tests', 'hostemu'))
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.fail('no clang for the host build of the kernel')
  lib = hb.build('clang', False, True, [], False, False, 'san')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'),
             ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:detect_stack_use_after_return=0:halt_on_error=1',
             UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
  env['LD_PRELOAD'] = os.pathsep.join([hb.preload('clang')] + ([os.environ['LD_PRELOAD']] if os.environ.get('LD_PRELOAD') else []))
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-q', '-p', 'no:cacheprovider'],
                     env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
  tail = r.stdout[-3000:] + r.stderr[-3000:]
  assert r.returncode == 0, tail
  assert 'Sanitizer' not in r.stdout + r.stderr and 'runtime error' not in r.stdout + r.stderr, tail
  summary = r.stdout.strip().splitlines()[-1]
  passed = re.search(r'(\d+) passed', summary)
  assert passed and int(passed.group(1)) == len(CASES) and 'skipped' not in summary and 'failed' not in summary, summary

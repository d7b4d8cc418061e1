"""Directed Doggo states for tests/test_doggo_branches.py and the census of the constraint rows a step STARTS from.

The Doggo kernel (csrc/sag_doggo_coop.hpp: joint-limit rows, the floor points, dc_collide_body, the tether row, the 32-lane
and the 64-lane solver) is reached by sampled layouts only where a rollout happens to touch something.  Here every env's
vases, pillars, buttons and task object are placed AROUND a robot in a known pose, each against a named robot geom at a
drawn depth of 1 - 8 mm (the contacts are stiff: deeper ones part the two oracle builds), and the census says which
branches those states reach.

  settled_pose(oracle)                -> the reset pose of golden_util.doggo_record after eight zero-action steps, fp32
  directed_records(name, n, base, oracle, settled) -> (rf, ri) of case `name`
  census(oracle, rf, ri)              -> Census of ONE record
  reach(name, tally)                  -> rows (what, occurrences, minimum) the case must reach

The census takes its contacts from the oracle's own list (oracle_lib.Oracle.doggo_contacts, keys decoded by
oracle_lib.decode_contact_key: the analytic tests of tests/test_oracle_doggo.py pin both), counts the joint-limit rows from q against
JOINT_RANGE_DEG (doggo.xml) and the tether from haul_box.py:21-29; rows = limits + 3 x contacts + taut.  It names what a
state reaches and is never the expected value of a step: that is the oracle's step."""
import collections
import math

import numpy as np

import contact_ref as cr
import oracle_lib as ol
from golden_util import doggo_record

EXT = ol.F_ROBOT_EXT
DOGGO = 2
N_ENVS, N_STEPS = 97, 3     # an odd batch: the last wavefront has an idle half
FAST_ROWS, ROW_BUDGET = 32, 50   # rows of the 32-lane path; rows an env may have on the device (more are dropped and flagged)

# doggo.xml joint ranges in the record's order: leg 1 (hip_z, hip_y, ankle), leg 4, waist, leg 2, leg 3
JOINT_RANGE_DEG = np.array([[-10, 30], [-75, 15], [-75, 0], [-10, 30], [-75, 15], [-75, 0], [-30, 30],
                            [-10, 30], [0, 135], [-75, 0], [-10, 30], [0, 135], [-75, 0]], np.float64)


def joint_range():
  """(lower, upper) joint limits in radians."""
  return np.radians(JOINT_RANGE_DEG[:, 0]), np.radians(JOINT_RANGE_DEG[:, 1])


GEOM_R = np.array([.075, .032, .032, .032, .032, .032, .032, .075, .032, .032, .032, .032, .032, .032])
CYLINDERS = (0, 7)                       # the two torso cylinders; every other collision geom is a capsule
AUX, HIPS, ANKLES = (1, 2, 8, 9), (3, 5, 10, 12), (4, 6, 11, 13)
RIM_POINTS, KNEE_POINTS, FOOT_POINTS = (0, 1, 8, 9), (3, 6, 11, 14), (4, 7, 12, 15)
SITE_R = 0.036                           # doggo.xml:8
MAX_PILLARS, MAX_BUTTONS, MAX_VASES = 2, 6, 10
OBJ_BUTTON0, OBJ_VASE0, OBJ_TASK = MAX_PILLARS, MAX_PILLARS + MAX_BUTTONS, MAX_PILLARS + MAX_BUTTONS + MAX_VASES
TASK_HAUL_BOX = 7
TETHER_RANGE, TETHER_Z = 0.75, 0.2       # haul_box.py:21-29
BOX_TOP = {cr.BOX_BOX: 0.4, cr.BOX_ROD: 0.16, cr.BOX_BALL: 0.28}
DEPTH_MAX = 0.009                        # no contact of a start state is deeper

ObjContact = collections.namedtuple('ObjContact', 'cls obj bg k g robot_kind obj_kind crosses above site depth')
Census = collections.namedtuple('Census', 'lower upper floor objects taut rows path cost_contacts')


def obj_class(obj):
  return 'pillar' if obj < OBJ_BUTTON0 else 'button' if obj < OBJ_VASE0 else 'vase' if obj < OBJ_TASK else 'object'


def obj_top(rf, ri, obj):
  cls = obj_class(obj)
  return {'pillar': 1.0, 'button': 0.2, 'vase': 2.0 * float(rf[ol.F_VASE_SIZE])}.get(cls) or BOX_TOP[int(ri[ol.I_BOX_KIND])]


def robot_geoms(oracle, rf, ri):
  """(floor points [16, 3], geom axes [14, 6]) of one record, world frame."""
  geo = oracle.doggo_debug(oracle.env(np.asarray(rf, np.float32), ri))[2]
  return geo[:48].reshape(16, 3), geo[48:].reshape(14, 6)


def limit_rows(rf):
  """(joints below their range, joints above it) of one record."""
  ext = np.asarray(rf, np.float64)[EXT:EXT + 35]
  if ext[1:5] @ ext[1:5] < 0.25:         # a zero quaternion: the reset pose, joints 0 (sag.h)
    return 0, 0
  lo, hi = joint_range()
  q = ext[9:22]
  return int((q < lo).sum()), int((q > hi).sum())


def tether_taut(rf, ri):
  """None without a tether; else whether base site <-> box site (z .2) is longer than .75."""
  if ri[ol.I_TASK] != TASK_HAUL_BOX or not ri[ol.I_BOX_KIND]:
    return None
  rf = np.asarray(rf, np.float64)
  fresh = rf[EXT + 1:EXT + 5] @ rf[EXT + 1:EXT + 5] < 0.25
  dx, dy, dz = rf[ol.F_BOX] - rf[0], rf[ol.F_BOX + 1] - rf[1], TETHER_Z - (0.22 if fresh else rf[EXT])
  d2 = dx * dx + dy * dy
  return bool(math.sqrt(d2 + dz * dz) > TETHER_RANGE and d2 >= 1e-18)


def census(oracle, rf, ri):
  rf32 = np.asarray(rf, np.float32)
  e = oracle.env(rf32, ri)
  rows, cc = oracle.doggo_contacts(e)
  ax = oracle.doggo_debug(e)[2][48:].reshape(14, 6)
  floor, objects = [], []
  for r in rows:
    kind, what = ol.decode_contact_key(r[0])
    if kind == 'floor':
      floor.append(int(what))
      continue
    obj, bg, k, g = what
    A, B = ax[g, :3], ax[g, 3:]
    top = obj_top(rf32, ri, obj)
    a_in, b_in = A[2] <= top, B[2] <= top
    cls = obj_class(obj)
    circle = cls in ('pillar', 'button') or (cls == 'object' and ri[ol.I_BOX_KIND] == cr.BOX_BALL)
    if g in CYLINDERS:                    # the rectangle under [t0, t1] of the axis: its middle decides the cross-section
      t0, t1 = 0.0, 1.0
      if a_in != b_in:
        tc = (top - A[2]) / (B[2] - A[2])
        t0, t1 = (0.0, tc) if a_in else (tc, 1.0)
      above = A[2] + 0.5 * (t0 + t1) * (B[2] - A[2]) > top
    else:
      above = r[3] > top                  # a capsule's contact is at the height of its axis point
    site = None
    if g in ANKLES:
      p = r[1:4]
      site = 'knee' if (p - A) @ (p - A) <= SITE_R ** 2 else 'foot' if (p - B) @ (p - B) <= SITE_R ** 2 else None
    objects.append(ObjContact(cls, obj, bg, k, g, 'cylinder' if g in CYLINDERS else 'capsule', 'circle' if circle else 'box',
                              bool(a_in != b_in), bool(above), site, float(r[7])))
  lower, upper = limit_rows(rf32)
  taut = tether_taut(rf32, ri)
  n = lower + upper + 3 * (len(floor) + len(objects)) + bool(taut)
  path = 'fast' if n <= FAST_ROWS else 'wide' if n <= ROW_BUDGET else 'overflow'
  return Census(lower, upper, floor, objects, taut, n, path, cc)


# ---- the planar aftermath of a push -------------------------------------------------------------------------------
def aftermath(rf, ri, cen):
  """Counts at one state: moving vases that overlap (another vase, a pillar or button, the task object), and sleeping
  vases within the kernel's reach of the robot (.6 m + the vase's bounding radius) that the robot does not touch."""
  rf = np.asarray(rf)
  nv = int(ri[ol.I_NV])
  vel = [bool(np.any(rf[ol.F_VASES + 6 * k + 3:ol.F_VASES + 6 * k + 6] != 0)) for k in range(nv)]
  out = collections.Counter()
  if any(vel):
    for o in cr.census(rf, ri, 'point').overlaps:     # (the planar pairs; the robot's own are the Doggo census')
      if o.a != 'vase' or o.depth <= 0:
        continue
      if o.b == 'vase' and (vel[o.ia] or vel[o.ib]):
        out['after_vase'] += 1
      elif o.b in ('pillar', 'button') and vel[o.ia]:
        out['after_static'] += 1
      elif o.b == 'object' and vel[o.ia]:
        out['after_object'] += 1
  touched = {c.obj - OBJ_VASE0 for c in cen.objects if c.cls == 'vase'}
  reach_r = 0.6 + math.sqrt(2) * float(rf[ol.F_VASE_SIZE])
  for k in range(nv):
    d = math.hypot(rf[ol.F_VASES + 6 * k] - rf[0], rf[ol.F_VASES + 6 * k + 1] - rf[1])
    if not vel[k] and not (ri[ol.I_AWAKE] >> k & 1) and k not in touched and d <= reach_r:
      out['sleeper'] += 1
  return out


class Tally:
  """The censuses of the states the steps of one case started from, plus the test's own counts (button events)."""

  def __init__(self):
    self.start = []                       # (step, env, Census)
    self.after = collections.Counter()    # aftermath() over the states of steps 2 onward
    self.events = 0                       # envs whose button contact changed I_BTN_STATE, I_ACTIVE_MASK or met the goal

  def add(self, step, cens, rf, ri, want_aftermath):
    self.start += [(step, e, c) for e, c in enumerate(cens)]
    if step >= 1 and want_aftermath:
      for e, c in enumerate(cens):
        self.after.update(aftermath(rf[e], ri[e], c))

  def states(self, pred, step=None):
    return sum(1 for t, _, c in self.start if (step is None or t == step) and pred(c))

  def contacts(self, pred):
    return sum(1 for _, _, c in self.start for o in c.objects if pred(o))

  def floor(self, points):
    return sum(1 for _, _, c in self.start for s in c.floor if s in points)

  def wide_twice(self):
    wide = [{e for t, e, c in self.start if t == s and c.path == 'wide'} for s in (0, 1)]
    return len(wide[0] & wide[1])


ROWS = {
    'fast': ('start states on the 32-lane path', lambda T: T.states(lambda c: c.path == 'fast', 0)),
    'wide': ('start states on the 64-lane path (33 - 50 rows)', lambda T: T.states(lambda c: c.path == 'wide', 0)),
    'both': ('the rarer of the two paths in the one batch', lambda T: min(T.states(lambda c: c.path == 'fast', 0), T.states(lambda c: c.path == 'wide', 0))),
    'wide_step2': ('envs on the 64-lane path at the start of steps 1 AND 2 (warm across a whole step)', lambda T: T.wide_twice()),
    'lower': ('joint-limit rows at a lower bound', lambda T: sum(c.lower for _, _, c in T.start)),
    'upper': ('joint-limit rows at an upper bound', lambda T: sum(c.upper for _, _, c in T.start)),
    'floor_sphere': ('floor: a foot\'s end sphere', lambda T: T.floor(FOOT_POINTS)),
    'floor_rim': ('floor: a torso cylinder\'s rim', lambda T: T.floor(RIM_POINTS)),
    'floor_knee': ('floor: a merged knee row', lambda T: T.floor(KNEE_POINTS)),
    'capsule_box': ('capsule x box', lambda T: T.contacts(lambda o: (o.robot_kind, o.obj_kind) == ('capsule', 'box'))),
    'capsule_circle': ('capsule x circle', lambda T: T.contacts(lambda o: (o.robot_kind, o.obj_kind) == ('capsule', 'circle'))),
    'cylinder_box': ('cylinder x box', lambda T: T.contacts(lambda o: (o.robot_kind, o.obj_kind) == ('cylinder', 'box'))),
    'cylinder_circle': ('cylinder x circle', lambda T: T.contacts(lambda o: (o.robot_kind, o.obj_kind) == ('cylinder', 'circle'))),
    'crosses': ('a geom axis that crosses the object\'s top', lambda T: T.contacts(lambda o: o.crosses)),
    'above': ('a contact above the top, through the reduced cross-section', lambda T: T.contacts(lambda o: o.above)),
    'site_knee': ('an object contact inside a knee site', lambda T: T.contacts(lambda o: o.site == 'knee')),
    'site_foot': ('an object contact inside a foot site', lambda T: T.contacts(lambda o: o.site == 'foot')),
    'pillar': ('pillar contacts', lambda T: T.contacts(lambda o: o.cls == 'pillar')),
    'button': ('button contacts', lambda T: T.contacts(lambda o: o.cls == 'button')),
    'button_event': ('envs whose button contact changed I_BTN_STATE, I_ACTIVE_MASK or met the goal', lambda T: T.events),
    'vase': ('vase contacts', lambda T: T.contacts(lambda o: o.cls == 'vase')),
    'box': ('task-object contacts (box, rod or ball)', lambda T: T.contacts(lambda o: o.cls == 'object')),
    'box_corner': ('contacts with the box\'s corner columns', lambda T: T.contacts(lambda o: o.cls == 'object' and o.bg >= 1)),
    'taut': ('start states with the tether taut', lambda T: T.states(lambda c: c.taut is True)),
    'slack': ('start states with the tether slack', lambda T: T.states(lambda c: c.taut is False)),
    'after_vase': ('steps 2 on: a moving vase overlapping another vase', lambda T: T.after['after_vase']),
    'after_static': ('steps 2 on: a moving vase overlapping a pillar or button', lambda T: T.after['after_static']),
    'after_object': ('steps 2 on: a moving vase overlapping the task object', lambda T: T.after['after_object']),
    'sleeper': ('steps 2 on: a sleeping vase within reach that stays asleep', lambda T: T.after['sleeper']),
}
# 'box' stands for the push_box box, the rod and the ball by case; the reach table names them apart
ROW_ALIAS = {'rod': 'box', 'ball': 'box', 'press_event': 'button_event', 'collect_event': 'button_event'}


# ---- the cases ----------------------------------------------------------------------------------------------------
# objects: (class, spec) in record order per class.  spec:
#   ('at', geoms, (t lo, t hi), probability)  against one of those robot geoms at axis parameter t, from either side, at any yaw
#   ('waist', probability)                    against both torso cylinders from one side, as the analytic waist scenario
#   ('far',)                                  a sleeping neighbour .50 - .56 m from the base
#   ('beyond', k)                             a corner (or the circle) 3 mm inside the far face of vase k: every third env the next
#                                             vase, the pillar, the task object in turn; it sleeps until the robot's push arrives
#   ('tether',) / ('tether', 'loose')         the haul_box box: odd envs 1 - 8 mm beyond the tether's range, even ones against a leg /
#                                             slack and clear of the robot
# Probability < 1: the object is otherwise put out of reach (50 m away).
LEGS = HIPS + ANKLES
CASES = {
    'legs_vases': dict(task='go_to_goal', pose='settled', reach=('fast', 'capsule_box', 'site_knee', 'site_foot', 'vase', 'floor_sphere', 'sleeper'),
                       objects=[('vase', ('at', ANKLES, (0.0, 0.12), 1.0)), ('vase', ('at', ANKLES, (0.85, 1.0), 1.0)), ('vase', ('far',))]),
    'torso_vases': dict(task='go_to_goal', pose='settled', reach=('fast', 'wide', 'both', 'wide_step2', 'cylinder_box', 'vase'),
                        objects=[('vase', ('waist', 0.8)), ('vase', ('at', CYLINDERS, (0.1, 0.9), 0.4)), ('vase', ('at', LEGS, (0.2, 0.8), 0.5))]),
    'pillars': dict(task='go_to_goal', pose='settled', reach=('pillar', 'capsule_circle'),
                    objects=[('pillar', ('at', LEGS + AUX, (0.0, 1.0), 1.0)), ('pillar', ('at', LEGS + AUX, (0.0, 1.0), 0.5))]),
    'press_buttons': dict(task='press_buttons', pose='settled', reach=('button', 'press_event', 'capsule_circle', 'cylinder_circle'),
                          objects=[('button', ('at', LEGS, (0.0, 1.0), 0.8)), ('button', ('waist', 0.5)),
                                   ('button', ('at', LEGS, (0.0, 1.0), 0.4)), ('button', ('at', AUX, (0.0, 1.0), 0.4))]),
    'collect': dict(task='collect', pose='settled', reach=('button', 'collect_event'),
                    objects=[('button', ('at', LEGS, (0.0, 1.0), 0.8)), ('button', ('at', CYLINDERS, (0.0, 1.0), 0.4)),
                             ('button', ('at', LEGS, (0.0, 1.0), 0.4)), ('button', ('at', AUX, (0.0, 1.0), 0.4))]),
    'push_box': dict(task='push_box', pose='settled', reach=('box', 'box_corner'),
                     objects=[('object', ('at', LEGS, (0.0, 1.0), 1.0)), ('vase', ('at', LEGS, (0.0, 1.0), 0.5))]),
    'roll_rod': dict(task='roll_rod', pose='settled', reach=('rod',),
                     objects=[('object', ('at', ANKLES, (0.3, 1.0), 1.0)), ('vase', ('at', LEGS, (0.0, 1.0), 0.5))]),
    'dribble_ball': dict(task='dribble_ball', pose='settled', reach=('ball', 'capsule_circle'),
                         objects=[('object', ('at', LEGS + CYLINDERS, (0.0, 1.0), 1.0)), ('vase', ('at', LEGS, (0.0, 1.0), 0.5))]),
    'haul_box': dict(task='haul_box', pose='settled', reach=('taut', 'slack', 'box'),
                     objects=[('object', ('tether',)), ('vase', ('at', LEGS, (0.0, 1.0), 0.7))]),
    'lying': dict(task='go_to_goal', pose='lying', reach=('floor_knee', 'floor_rim', 'vase'),
                  objects=[('vase', ('at', CYLINDERS + HIPS, (0.1, 0.9), 0.8))]),
    # (every leg points forward: beside the waist a pillar, r .2, is 4 - 6 cm inside the rear legs; buttons, r .1, reach the torso)
    'falling': dict(task='press_buttons', pose='reset', reach=('crosses', 'above', 'button', 'vase'),
                    objects=[('vase', ('at', HIPS, (0.1, 0.9), 0.9)), ('vase', ('at', AUX + CYLINDERS, (0.1, 0.9), 0.9)),
                             ('button', ('at', HIPS, (0.1, 0.9), 0.7))]),
    'joint_limits': dict(task='go_to_goal', pose='limits', reach=('lower', 'upper', 'floor_sphere'),
                         objects=[('vase', ('at', LEGS, (0.0, 1.0), 0.5))]),
    'vase_chain': dict(task='push_box', pose='settled', reach=('after_vase', 'after_static', 'after_object', 'sleeper', 'vase'),
                       objects=[('vase', ('at', ANKLES, (0.3, 0.9), 1.0)), ('vase', ('beyond', 0)), ('pillar', ('beyond', 0)),
                                ('object', ('beyond', 0)), ('vase', ('far',))]),
}
OVERFLOW = 'overflow'                      # not stepped: 45 - 60 rows, vases all round the settled robot
CASES_ALL = dict(CASES, **{OVERFLOW: dict(task='haul_box', pose='settled8', reach=(),
                                          objects=[('object', ('tether', 'loose')), ('vase', ('waist', 1.0)), ('vase', ('waist', 0.5))] +
                                          [('vase', ('at', ANKLES, (0.2, 0.8), 0.5))] * 3)})
CASE_SEED = {name: 7100 + 13 * k for k, name in enumerate(CASES_ALL)}
FAR = 50.0


def reach(name, tally):
  """Rows (what, occurrences, minimum) case `name` must reach over the states its steps started from."""
  return [(ROWS[ROW_ALIAS.get(k, k)][0] + (f' [{k}]' if k in ROW_ALIAS else ''), ROWS[ROW_ALIAS.get(k, k)][1](tally), 5)
          for k in CASES[name]['reach']]


def settled_pose(oracle):
  """The reset pose (z .22, joints 0) after eight zero-action steps of the fp64 oracle: standing at rest, as fp32."""
  rf, ri = doggo_record()
  e = oracle.env(rf, ri)
  for _ in range(8):
    oracle.step(e, DOGGO, np.zeros(12), noise=np.zeros(12))
  return oracle.record(e, f64=False)[0]


def _qmul(a, b):
  w0, x0, y0, z0 = a
  w1, x1, y1, z1 = b
  return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                   w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])


def _pose(kind, rs, settled, e):
  """(robot6 relative to the env's own xy, ext[35]) of one env."""
  rob, ext = np.zeros(6), np.zeros(35)
  if kind in ('settled', 'limits', 'settled8'):
    rob[:], ext[:] = settled[0:6], settled[EXT:EXT + 35]
    if kind == 'settled8' and (e % 2 == 0 or e % 8 == 1):   # two hip_z joints (vertical axes: the feet stay on the floor) below their range: 8 limit rows
      lo, _ = joint_range()
      for j in rs.choice([0, 3, 7, 10], 2, replace=False):
        ext[9 + j] = lo[j] - rs.uniform(0.002, 0.01)
    if kind == 'limits':                  # three joints up to .02 rad beyond a bound, lower and upper in turn
      lo, hi = joint_range()
      for n, j in enumerate(rs.choice(13, 3, replace=False)):
        beyond = rs.uniform(0.002, 0.02)
        ext[9 + j] = lo[j] - beyond if (n + e) % 2 else hi[j] + beyond
  elif kind == 'reset':
    ext[0], ext[1] = 0.22, 1.0
  elif kind == 'lying':                   # even envs on the left side on the knees of legs 1 and 2, odd ones on the back on the torso
    if e % 2 == 0:
      ext[0] = 0.1566 + 0.032 - rs.uniform(0.001, 0.006)
      ext[1:5] = [math.cos(-math.pi / 4), math.sin(-math.pi / 4), 0, 0]
    else:
      pitch = rs.uniform(-0.015, 0.015)
      ext[0] = 0.075 - rs.uniform(0.001, 0.004)
      ext[1:5] = _qmul([0, 1, 0, 0], [math.cos(pitch / 2), 0, math.sin(pitch / 2), 0])
  return rob, ext


def _against(ax, g, t, side, depth, top, shape, size, yaw):
  """Centre of a circle (radius `size`) or of a box (half sizes `size`, at `yaw`) that meets robot geom g `depth` deep at
  axis parameter t, from the side `side` of the axis in plan view; None where the geom is out of reach above the top."""
  A, B = ax[g, :3], ax[g, 3:]
  P = A + t * (B - A)
  d = (B - A)[:2]
  L = math.hypot(*d)
  u = d / L if L > 1e-6 else np.array([1.0, 0.0])
  out = side * np.array([-u[1], u[0]])
  r = GEOM_R[g]
  if P[2] > top:
    q = r * r - (P[2] - top) ** 2
    if q <= 1e-5:
      return None
    r = math.sqrt(q)
  if shape == 'circle':
    return P[:2] + (r + size - depth) * out
  c, s = math.cos(yaw), math.sin(yaw)
  corners = [np.array([c * sx * size[0] - s * sy * size[1], s * sx * size[0] + c * sy * size[1]]) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
  k = int(np.argmin([v @ out for v in corners]))
  return P[:2] + (r - depth) * out - corners[k]


def _place(spec, cls, rs, rf, ri, ax, placed):
  """(x, y, yaw) of one object of class cls, or None to put it out of reach."""
  base = np.asarray(rf[0:2], np.float64)
  vs = float(rf[ol.F_VASE_SIZE])
  kind = int(ri[ol.I_BOX_KIND])
  shape = 'circle' if cls in ('pillar', 'button') or (cls == 'object' and kind == cr.BOX_BALL) else 'box'
  size = {'pillar': float(rf[ol.F_PILLAR_SIZE]), 'button': cr.BUTTON_R, 'vase': (vs, vs)}.get(cls)
  if cls == 'object':
    size = {cr.BOX_BOX: (0.3, 0.3), cr.BOX_ROD: (0.08, 0.3), cr.BOX_BALL: 0.14}[kind]   # (the box with its corner columns spans .3)
  top = {'pillar': 1.0, 'button': 0.2, 'vase': 2 * vs}.get(cls) or BOX_TOP[kind]
  yaw = rs.uniform(0, 2 * math.pi)
  if spec[0] == 'far':
    d, th = rs.uniform(0.50, 0.56), rs.uniform(0, 2 * math.pi)
    return (*(base + d * np.array([math.cos(th), math.sin(th)])), yaw)
  if spec[0] == 'tether':                 # every other env beyond the range by 1 - 8 mm, the others against a leg
    taut = placed['env'] % 2 == 1
    if not taut and len(spec) > 1:        # ('tether', 'loose'): slack and clear of the robot
      d, th = rs.uniform(0.70, 0.745), rs.uniform(0, 2 * math.pi)
      return (*(base + d * np.array([math.cos(th), math.sin(th)])), th)   # (a face towards the robot: .4 m away)
    if taut:
      dz = TETHER_Z - float(rf[EXT])
      d, th = math.sqrt((TETHER_RANGE + rs.uniform(0.001, 0.008)) ** 2 - dz * dz), rs.uniform(0, 2 * math.pi)
      return (*(base + d * np.array([math.cos(th), math.sin(th)])), th)     # (a face towards the robot, clear of its legs)
    spec = ('at', LEGS, (0.0, 1.0), 1.0)
  if spec[0] == 'waist':                  # against both torso cylinders from one side, as the analytic waist scenario (a face, or a circle)
    if rs.uniform() >= spec[1]:
      return None
    A, B = ax[0, :2], ax[0, 3:5]
    u = (B - A) / np.linalg.norm(B - A)
    side = 1.0 if rs.uniform() < 0.5 else -1.0
    if placed.get('waist'):
      side = -placed['waist']             # a second one takes the other side
    placed['waist'] = side
    out = side * np.array([-u[1], u[0]])
    half = size if shape == 'circle' else size[0]
    c = A + rs.uniform(-0.02, 0.05) * u + (GEOM_R[0] + half - rs.uniform(0.001, 0.006)) * out
    return (c[0], c[1], math.atan2(u[1], u[0]))
  if spec[0] == 'beyond':
    vx, vy, vyaw, out = placed['vase'][spec[1]]
    which = ('vase', 'pillar', 'object')[placed['env'] % 3]
    if cls != which:
      return None
    face = np.array([vx, vy]) + (vs - 0.003) * out + np.array([-out[1], out[0]]) * rs.uniform(-0.04, 0.04)   # 3 mm inside the far face
    if shape == 'circle':
      return (*(face + size * out), 0.0)
    nyaw = vyaw + rs.uniform(0.1, 0.6)    # a corner first: two boxes face to face are a degenerate pair
    h = size if cls == 'vase' else (0.3, 0.3)   # (the box's corner columns end at .3)
    c, s = math.cos(nyaw), math.sin(nyaw)
    corners = [np.array([c * sx * h[0] - s * sy * h[1], s * sx * h[0] + c * sy * h[1]]) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    return (*(face - corners[int(np.argmin([v @ out for v in corners]))]), nyaw)
  _, geoms, (tlo, thi), prob = spec
  if rs.uniform() >= prob:
    return None
  g = geoms[rs.randint(len(geoms))]
  side = 1.0 if rs.uniform() < 0.5 else -1.0
  depth = rs.uniform(0.001, 0.008)
  A, B = ax[g, :2], ax[g, 3:5]
  u = B - A
  u = u / max(np.linalg.norm(u), 1e-9)
  out = side * np.array([-u[1], u[0]])
  if placed.get('chain'):                 # the pushed vase of a chain turns a face away from the robot (not squarely: a face parallel to
    yaw = math.atan2(out[1], out[0]) + rs.uniform(0.1, 0.3) * (1 if rs.uniform() < 0.5 else -1)   # the capsule's axis is a degenerate pair)
  c = _against(ax, g, rs.uniform(tlo, thi), side, depth, top, shape, size, yaw)
  if c is None:
    return None
  placed.setdefault(cls, []).append((c[0], c[1], yaw, np.array([math.cos(yaw), math.sin(yaw)]) if placed.get('chain') else out))
  return (c[0], c[1], yaw)


def _write(rf, cls, k, pos):
  if cls == 'vase':
    rf[ol.F_VASES + 6 * k:ol.F_VASES + 6 * k + 3] = pos
  elif cls == 'pillar':
    rf[ol.F_PILLARS + 2 * k:ol.F_PILLARS + 2 * k + 2] = pos[:2]
  elif cls == 'button':
    rf[ol.F_BUTTONS + 2 * k:ol.F_BUTTONS + 2 * k + 2] = pos[:2]
  else:
    rf[ol.F_BOX:ol.F_BOX + 3] = pos


def directed_records(name, n, base, oracle, settled):
  """The directed state of case `name`: base = (rf, ri), n sampled records of the case's task (their xy, goal, sizes and
  task ints are kept).  Every env gets the case's robot pose at its own xy and its objects against that robot's geoms; an
  object is redrawn while it makes a contact deeper than DEPTH_MAX (and left out after 40 draws), an env until its rows fit the
  device's budget with room to spare (the overflow case: until it has 45 - 60 rows).
  Everything is at rest; which bodies sleep is left to the install.  Returns (rf, ri)."""
  spec = CASES_ALL[name]
  rs = np.random.RandomState(CASE_SEED[name])
  rf, ri = np.array(base[0], np.float32), np.array(base[1], np.int32)
  assert len(rf) == n
  counts = collections.Counter(cls for cls, _ in spec['objects'])
  for e in range(n):
    ri[e, ol.I_NH] = 0
    ri[e, ol.I_NV], ri[e, ol.I_NP] = counts['vase'], counts['pillar']
    if counts['button']:
      ri[e, ol.I_NB] = counts['button']
      ri[e, ol.I_GOAL_BUTTON] %= counts['button']
      ri[e, ol.I_BTN_STATE] = 1
      ri[e, ol.I_ACTIVE_MASK] &= (1 << counts['button']) - 1
      if spec['task'] == 'collect' and not ri[e, ol.I_ACTIVE_MASK]:
        ri[e, ol.I_ACTIVE_MASK] = 1
    else:
      ri[e, ol.I_NB] = 0
    rf[e, ol.F_HAZARDS:ol.F_HAZARDS + 18] = FAR
    for attempt in range(2000):
      rf[e, ol.F_PILLARS:ol.F_PILLARS + 4] = FAR
      rf[e, ol.F_BUTTONS:ol.F_BUTTONS + 12] = FAR
      rf[e, ol.F_VASES:ol.F_VASES + 60] = 0
      for k in range(counts['vase']):
        rf[e, ol.F_VASES + 6 * k:ol.F_VASES + 6 * k + 2] = [FAR + 2 * k, FAR]
      if ri[e, ol.I_BOX_KIND]:
        rf[e, ol.F_BOX:ol.F_BOX + 6] = [FAR, FAR, 0, 0, 0, 0]
      rob, ext = _pose(spec['pose'], rs, settled, e)
      rf[e, 2:6], rf[e, EXT:EXT + 35] = rob[2:6], ext
      if spec['pose'] in ('lying', 'reset'):
        rf[e, 2] = 0
      _, ax = robot_geoms(oracle, rf[e], ri[e])
      placed = {'env': e, 'chain': name == 'vase_chain'}
      idx = collections.Counter()
      for cls, sp in spec['objects']:
        k = idx[cls]
        idx[cls] += 1
        far = (FAR + 2 * k, FAR + {'vase': 0, 'pillar': 10, 'button': 20, 'object': 30}[cls], 0.0)   # out of reach, apart from each other
        for tries in range(40):           # the object alone is redrawn while it makes a contact deeper than DEPTH_MAX
          keep = {key: (list(v) if isinstance(v, list) else v) for key, v in placed.items()}
          pos = _place(sp if tries < 39 or sp[0] != 'tether' else ('tether', 'loose'), cls, rs, rf[e], ri[e], ax, placed)   # (a tethered box is never left out)
          _write(rf[e], cls, k, pos or far)
          if pos is None or max([o.depth for o in census(oracle, rf[e], ri[e]).objects], default=0.0) <= DEPTH_MAX:
            break
          placed.clear()
          placed.update(keep)
          _write(rf[e], cls, k, far)
      c = census(oracle, rf[e], ri[e])
      deepest = max([o.depth for o in c.objects], default=0.0)
      if name == OVERFLOW:
        # every eighth env: full with the tether slack (8 limits + 3 x 14 contacts); the next: full BEFORE its taut tether, whose
        # row is then the only one that does not fit (51 rows)
        want = ROW_BUDGET if e % 8 == 0 else ROW_BUDGET + 1 if e % 8 == 1 else None
        if deepest <= DEPTH_MAX and (c.rows == want if want else 45 <= c.rows <= 60):
          break
      elif deepest <= DEPTH_MAX and c.rows <= ROW_BUDGET - 6:   # (six rows of room: a push may add two contacts)
        break
    else:
      raise AssertionError(f'{name}: env {e} found no admissible placement')
  import reset_sampler_ref as R           # what an install derives: task.reset's `last` distances, the awake word
  rf[:, ol.F_LAST:ol.F_LAST + 3] = R.install_last(rf, ri)
  ri[:, ol.I_AWAKE] = R.install_awake(rf, ri)
  return rf, ri


def step_inputs(rng, n):
  """(actions, zero action noise, tape) of one step: uniform random actions, the lockstep's random tape."""
  act = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
  tape = rng.randint(0, 2**32, size=(n, 64), dtype=np.uint32)
  return act, np.zeros((n, 12), np.float32), tape


def discrete(done, met, used, ints):
  """done, goal_met, words used and the task ints of a batch as one integer table."""
  return np.concatenate([done[:, None], met[:, None], used[:, None], ints], 1).astype(np.int64)


def button_events(ri0, ri1, met):
  """Envs whose step changed I_BTN_STATE or I_ACTIVE_MASK or met the goal."""
  return (met != 0) | (ri1[:, ol.I_BTN_STATE] != ri0[:, ol.I_BTN_STATE]) | (ri1[:, ol.I_ACTIVE_MASK] != ri0[:, ol.I_ACTIVE_MASK])

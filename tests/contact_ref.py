"""A float64 census of the planar contacts a step STARTS from, and the generator of the dense directed states of
tests/test_contact_branches.py.

The census restates the footprints and the three pair tests of DESIGN.md section 4 ("circle/box narrowphase (closest
point; box-box by vertices strictly inside the other box, least-penetration face)") from the specification and the values
it cites - point.xml:18-19, car.xml:16-32, primitive_objects.py (vases), push_box.py:28-72, roll_rod.py:19-43,
dribble_ball.py:18-41, press_buttons.py:16 - not from the kernels.  It says WHICH branch of the narrow phase a pose
reaches (and how deep), so that a test can prove what its states exercise.  It is never the expected value of a step:
that is the oracle's.

  census(rf, ri, robot) -> Census(overlaps, n_dynamic, taut)
  Overlap.key = (body class A, body class B, geom index A, geom index B, branch), with the depth attached

Branches: 'cc', 'cb-face', 'cb-corner', 'cb-centre-inside' (circle against box: the closest point on a face, at a corner,
or the circle's centre inside the box), 'bb' with verts = (vertices of A strictly inside B, vertices of B strictly inside
A).  Two boxes that overlap without a vertex of either inside the other (crossed edges) are listed as 'bb' (0, 0) at
depth 0: the specification makes no contact of them.  A and B follow the fixed pair order of the specification: robot -
pillars, robot - buttons, robot - vases, robot - object, vase - pillars, vase - buttons, object - pillars, object -
buttons, vase - vase (i < j), vase - object."""
import collections
import math

import numpy as np

from oracle_lib import (F_BOX, F_BUTTONS, F_HAZARDS, F_PILLAR_SIZE, F_PILLARS, F_ROBOT, F_VASE_SIZE, F_VASES, I_AWAKE,
                        I_BOX_KIND, I_BTN_STATE, I_GOAL_BUTTON, I_NB, I_NH, I_NP, I_NV, I_TASK)

MAX_VASES = 10
TASK_HAUL_BOX = 7
BOX_BOX, BOX_ROD, BOX_BALL = 1, 2, 3
BUTTON_R = 0.1                                   # press_buttons.py:16
TETHER_RANGE, TETHER_DZ = 0.75, 0.1              # haul_box.py:21-29: L = sqrt(d^2 + .1^2) <= .75
# The ball's centre is .04 above the Point sphere's: the two spheres (r .14 and .1) touch at the horizontal distance
# sqrt(.24^2 - .04^2), so the ball presents this radius to the sphere (and .14 to the arrow box, which spans its height)
BALL_TO_SPHERE = math.sqrt(0.24 ** 2 - 0.04 ** 2) - 0.1

# footprints: ('c', ox, oy, radius, -) or ('b', ox, oy, half x, half y) in the body frame
POINT = (('c', 0, 0, 0.1, 0), ('b', 0.1, 0, 0.05, 0.05))
CAR = (('b', 0, 0, 0.1, 0.1), ('b', 0, 0.15, 0.1, 0.01), ('b', 0, 0.125, 0.01, 0.025), ('b', 0, -0.165, 0.05, 0.01),
       ('b', 0, -0.13, 0.05, 0.03), ('b', -0.13, 0.1, 0.025, 0.05), ('b', 0.13, 0.1, 0.025, 0.05), ('c', 0, -0.1, 0.05, 0))
OBJECT = {BOX_BOX: (('b', 0, 0, 0.2, 0.2), ('b', 0.2, 0.2, 0.1, 0.1), ('b', -0.2, 0.2, 0.1, 0.1), ('b', 0.2, -0.2, 0.1, 0.1),
                    ('b', -0.2, -0.2, 0.1, 0.1)),
          BOX_ROD: (('b', 0, 0, 0.08, 0.3),),
          BOX_BALL: (('c', 0, 0, 0.14, 0),)}
ROBOT_GEOMS = {'point': POINT, 'car': CAR}

Overlap = collections.namedtuple('Overlap', 'a b ia ib ga gb branch verts depth')
Overlap.key = property(lambda o: (o.a, o.b, o.ga, o.gb, o.branch))
Census = collections.namedtuple('Census', 'overlaps n_dynamic taut')
Body = collections.namedtuple('Body', 'cls idx x y yaw geoms')


# ---- the three pair tests ----------------------------------------------------------------------------------------
def circle_circle(ax, ay, ra, bx, by, rb):
  """(branch, verts, depth) or None; touching is not a contact."""
  d = math.hypot(bx - ax, by - ay)
  return ('cc', None, ra + rb - d) if d < ra + rb else None


def circle_box(cx, cy, r, bx, by, yaw, hx, hy):
  c, s = math.cos(yaw), math.sin(yaw)
  wx, wy = cx - bx, cy - by
  lx, ly = c * wx + s * wy, -s * wx + c * wy
  ex, ey = abs(lx) - hx, abs(ly) - hy          # signed distances to the two pairs of faces
  if ex <= 0 and ey <= 0:                      # the centre inside the box (or on its boundary): the nearer face expels it
    return ('cb-centre-inside', None, r + min(-ex, -ey))
  d = math.hypot(max(ex, 0.0), max(ey, 0.0))
  if d >= r:
    return None
  return ('cb-corner' if ex > 0 and ey > 0 else 'cb-face', None, r - d)


def _corners(x, y, yaw, hx, hy):
  c, s = math.cos(yaw), math.sin(yaw)
  return [(x + c * sx * hx - s * sy * hy, y + s * sx * hx + c * sy * hy) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def verts_inside(px, py, pyaw, phx, phy, qx, qy, qyaw, qhx, qhy):
  """Depths (to the least-penetrated face of Q) of the vertices of box P strictly inside box Q."""
  c, s = math.cos(qyaw), math.sin(qyaw)
  out = []
  for vx, vy in _corners(px, py, pyaw, phx, phy):
    wx, wy = vx - qx, vy - qy
    dx, dy = qhx - abs(c * wx + s * wy), qhy - abs(-s * wx + c * wy)
    if dx > 0 and dy > 0:
      out.append(min(dx, dy))
  return out


def _sat_overlap(a, b):
  """Exact separating-axis test of two oriented boxes (x, y, yaw, hx, hy): True if their interiors meet."""
  for ref in (a, b):
    c, s = math.cos(ref[2]), math.sin(ref[2])
    for ux, uy in ((c, s), (-s, c)):
      span = []
      for box in (a, b):
        p = [vx * ux + vy * uy for vx, vy in _corners(*box)]
        span.append((min(p), max(p)))
      if span[0][1] <= span[1][0] or span[1][1] <= span[0][0]:
        return False
  return True


def box_box(ax, ay, ayaw, ahx, ahy, bx, by, byaw, bhx, bhy):
  va = verts_inside(ax, ay, ayaw, ahx, ahy, bx, by, byaw, bhx, bhy)
  vb = verts_inside(bx, by, byaw, bhx, bhy, ax, ay, ayaw, ahx, ahy)
  if va or vb:
    return ('bb', (len(va), len(vb)), max(va + vb))
  if _sat_overlap((ax, ay, ayaw, ahx, ahy), (bx, by, byaw, bhx, bhy)):
    return ('bb', (0, 0), 0.0)
  return None


def _geom_world(body, g):
  c, s = math.cos(body.yaw), math.sin(body.yaw)
  return body.x + c * g[1] - s * g[2], body.y + s * g[1] + c * g[2]


def geom_pair(A, ga, B, gb, ra=None, rb=None):
  """The pair test of geom ga of body A against geom gb of body B; ra / rb replace a circle's radius."""
  a, b = A.geoms[ga], B.geoms[gb]
  ax, ay = _geom_world(A, a)
  bx, by = _geom_world(B, b)
  if a[0] == 'c' and b[0] == 'c':
    return circle_circle(ax, ay, a[3] if ra is None else ra, bx, by, b[3] if rb is None else rb)
  if a[0] == 'c':
    return circle_box(ax, ay, a[3] if ra is None else ra, bx, by, B.yaw, b[3], b[4])
  if b[0] == 'c':
    return circle_box(bx, by, b[3] if rb is None else rb, ax, ay, A.yaw, a[3], a[4])
  return box_box(ax, ay, A.yaw, a[3], a[4], bx, by, B.yaw, b[3], b[4])


# ---- the census of one record ------------------------------------------------------------------------------------
def bodies(rf, ri, robot):
  """The bodies of one record by class: the robot, pillars, buttons, vases, the task object (or None)."""
  rf = np.asarray(rf, np.float64)
  R = Body('robot', 0, rf[F_ROBOT], rf[F_ROBOT + 1], rf[F_ROBOT + 2], ROBOT_GEOMS[robot])
  vs = rf[F_VASE_SIZE]
  P = [Body('pillar', k, rf[F_PILLARS + 2 * k], rf[F_PILLARS + 2 * k + 1], 0.0, (('c', 0, 0, rf[F_PILLAR_SIZE], 0),))
       for k in range(ri[I_NP])]
  B = [Body('button', k, rf[F_BUTTONS + 2 * k], rf[F_BUTTONS + 2 * k + 1], 0.0, (('c', 0, 0, BUTTON_R, 0),))
       for k in range(ri[I_NB])]
  V = [Body('vase', k, *rf[F_VASES + 6 * k:F_VASES + 6 * k + 3], (('b', 0, 0, vs, vs),)) for k in range(ri[I_NV])]
  O = Body('object', 0, *rf[F_BOX:F_BOX + 3], OBJECT[int(ri[I_BOX_KIND])]) if ri[I_BOX_KIND] else None
  return R, P, B, V, O


def census(rf, ri, robot):
  R, P, B, V, O = bodies(rf, ri, robot)
  ball = O is not None and ri[I_BOX_KIND] == BOX_BALL
  pairs = [(R, q) for q in P + B + V] + ([(R, O)] if O else [])
  pairs += [(v, q) for v in V for q in P + B]
  pairs += [(O, q) for q in P + B] if O else []
  pairs += [(V[i], V[j]) for i in range(len(V)) for j in range(i + 1, len(V))]
  pairs += [(v, O) for v in V] if O else []
  out = []
  for A, Bd in pairs:
    for ga in range(len(A.geoms)):
      for gb in range(len(Bd.geoms)):
        sphere_ball = ball and A is R and Bd is O and robot == 'point' and ga == 0
        hit = geom_pair(A, ga, Bd, gb, rb=BALL_TO_SPHERE if sphere_ball else None)
        if hit:
          out.append(Overlap(A.cls, Bd.cls, A.idx, Bd.idx, ga, gb, *hit))
  rf = np.asarray(rf)
  moving = [bool(np.any(rf[F_VASES + 6 * k + 3:F_VASES + 6 * k + 6] != 0)) for k in range(ri[I_NV])]
  n_dyn = sum(m or bool(ri[I_AWAKE] >> k & 1) for k, m in enumerate(moving))
  if O:
    n_dyn += bool(np.any(rf[F_BOX + 3:F_BOX + 6] != 0)) or bool(ri[I_AWAKE] >> MAX_VASES & 1)
  taut = None
  if ri[I_TASK] == TASK_HAUL_BOX and O:
    d = math.hypot(O.x - R.x, O.y - R.y)
    taut = math.sqrt(d * d + TETHER_DZ ** 2) > TETHER_RANGE
  return Census(out, int(n_dyn), taut)


def wake_chains(rf, ri, robot, overlaps):
  """Triples (i, j, k) of vases: i moves, j and k sleep (no velocity, no awake bit, not touched by the robot), i makes a
  contact with j and j with k: the pair walk wakes j, and the specification still skips j - k (both slept when it began)."""
  rf = np.asarray(rf)
  nv = int(ri[I_NV])
  moving = [bool(np.any(rf[F_VASES + 6 * k + 3:F_VASES + 6 * k + 6] != 0)) for k in range(nv)]
  touched = {o.ib for o in overlaps if o.a == 'robot' and o.b == 'vase' and o.depth > 0}
  asleep = [not moving[k] and not (ri[I_AWAKE] >> k & 1) and k not in touched for k in range(nv)]
  adj = {(o.ia, o.ib) for o in overlaps if o.a == 'vase' and o.b == 'vase' and o.depth > 0}
  adj |= {(j, i) for i, j in adj}
  return [(i, j, k) for i, j in adj if moving[i] and asleep[j] for k in range(nv) if k != i and (j, k) in adj and asleep[k]]


class Tally:
  """Counts of census keys over many records: count(...) selects by any part of the key."""

  def __init__(self):
    self.rows = []

  def add(self, overlaps):
    self.rows += [o for o in overlaps if o.depth > 0]

  def count(self, a=None, b=None, ga=None, gb=None, branch=None, verts=None, depth=0.0):
    sel = lambda want, got: want is None or (want(got) if callable(want) else got == want)   # noqa: E731
    return sum(1 for o in self.rows if sel(a, o.a) and sel(b, o.b) and sel(ga, o.ga) and sel(gb, o.gb) and
               sel(branch, o.branch) and sel(verts, o.verts) and o.depth > depth)


# ---- the directed states -----------------------------------------------------------------------------------------
# name: robot, task, vases, pillars, buttons, sleep (velocity on every other vase only, I_AWAKE = 0)
CASES = {
    'vase_crowd': ('point', 'go_to_goal', 8, 2, 0, False),
    'wake_order': ('point', 'go_to_goal', 8, 2, 0, True),
    'buttons': ('point', 'press_buttons', 3, 1, 4, False),
    'push_box': ('point', 'push_box', 4, 1, 0, False),
    'roll_rod': ('point', 'roll_rod', 4, 1, 0, False),
    'dribble_ball': ('point', 'dribble_ball', 4, 1, 0, False),
    'point_haul_box': ('point', 'haul_box', 4, 1, 0, False),
    'car_haul_box': ('car', 'haul_box', 4, 1, 0, False),
    'car_push_box': ('car', 'push_box', 4, 1, 0, False),
    'car_dribble_ball': ('car', 'dribble_ball', 4, 1, 0, False),
}
# distance windows from the robot, lower ends (the upper end is the env's `spread`, .35 - .5 m)
NEAR = {'pillar': 0.25, 'vase': 0.12, 'object': 0.25, 'ball': 0.15, 'button': 0.15}
CASE_SEED = {name: 9000 + 17 * k for k, name in enumerate(CASES)}


def directed_records(name, n, base):
  """The dense state of case `name`: base = (rf, ri), n valid records of the case's robot and task (their robot pose, goal,
  gear, scales and task ints are kept).  Every body of an env is placed around its robot - distance uniform in
  [NEAR[class], spread], bearing and yaw uniform - so that overlaps are the rule; free bodies move at up to .3 m/s and
  1 rad/s, the robot at up to .5 m/s; hazards sit at 50 m.  haul_box: the box of every other env at .76 - .95 m, beyond
  the tether's range (L = sqrt(d^2 + .01) > .75 from d = .7433).  Returns (rf, ri, awake): awake is the I_AWAKE word to
  give sag_set_state after the install (every body awake, or 0 for the wake-order case)."""
  robot, task, nv, np_, nb, sleep = CASES[name]
  rs = np.random.RandomState(CASE_SEED[name])
  rf, ri = np.array(base[0], np.float32), np.array(base[1], np.int32)
  assert len(rf) == n
  ri[:, I_NH], ri[:, I_NV], ri[:, I_NP], ri[:, I_NB] = 0, nv, np_, nb
  rf[:, F_HAZARDS:F_HAZARDS + 18] = 50.0
  rf[:, F_PILLARS:F_PILLARS + 4] = 50.0
  rf[:, F_BUTTONS:F_BUTTONS + 12] = 50.0
  rf[:, F_VASES:F_VASES + 60] = 0.0
  spread = rs.uniform(0.35, 0.5, n)
  rob = rf[:, F_ROBOT:F_ROBOT + 2].astype(np.float64)

  def around(lo, hi=None):
    d = rs.uniform(lo, spread if hi is None else hi)
    th = rs.uniform(0, 2 * np.pi, n)
    return rob + np.stack([d * np.cos(th), d * np.sin(th)], -1)

  def velocity(on=True):
    sp, th = rs.uniform(0, 0.3, n), rs.uniform(0, 2 * np.pi, n)
    v = np.stack([sp * np.cos(th), sp * np.sin(th), rs.uniform(-1, 1, n)], -1)
    return v * (1.0 if on else 0.0)

  sp, th = rs.uniform(0, 0.5, n), rs.uniform(0, 2 * np.pi, n)
  rf[:, F_ROBOT + 2] = rs.uniform(0, 2 * np.pi, n)
  rf[:, F_ROBOT + 3], rf[:, F_ROBOT + 4], rf[:, F_ROBOT + 5] = sp * np.cos(th), sp * np.sin(th), rs.uniform(-1, 1, n)
  for k in range(np_):
    rf[:, F_PILLARS + 2 * k:F_PILLARS + 2 * k + 2] = around(NEAR['pillar'])
  for k in range(nb):
    rf[:, F_BUTTONS + 2 * k:F_BUTTONS + 2 * k + 2] = around(NEAR['button'])
  for k in range(nv):
    rf[:, F_VASES + 6 * k:F_VASES + 6 * k + 2] = around(NEAR['vase'])
    rf[:, F_VASES + 6 * k + 2] = rs.uniform(0, 2 * np.pi, n)
    rf[:, F_VASES + 6 * k + 3:F_VASES + 6 * k + 6] = velocity(not sleep or k % 2 == 0)
  if nb:
    ri[:, I_GOAL_BUTTON] %= nb
    ri[:, I_BTN_STATE] = 1
  if ri[0, I_BOX_KIND]:
    ball = ri[0, I_BOX_KIND] == BOX_BALL
    pos = around(NEAR['ball' if ball else 'object'])
    if task == 'haul_box':
      far = around(0.76, 0.95)
      pos[1::2] = far[1::2]
    rf[:, F_BOX:F_BOX + 2] = pos
    rf[:, F_BOX + 2] = rs.uniform(0, 2 * np.pi, n)
    rf[:, F_BOX + 3:F_BOX + 6] = velocity()
  awake = 0 if sleep else (1 << nv) - 1 | (1 << MAX_VASES if ri[0, I_BOX_KIND] else 0)
  return rf, ri, awake


# ---- what each case must reach -----------------------------------------------------------------------------------
def reach(name, tally):
  """The case table: rows (what, occurrences, occurrences deeper than 1 mm, minimum) of the census keys case `name`
  must reach over the states its steps start from.  Counts per env (dynamic bodies, wake chains, the tether, button
  events) are the test's own rows."""
  c = lambda **kw: (tally.count(**kw), tally.count(depth=1e-3, **kw))   # noqa: E731
  cb = ('cb-face', 'cb-corner', 'cb-centre-inside')
  any_cb = lambda b: b in cb   # noqa: E731
  rows = []

  def need(what, minimum=5, **kw):
    rows.append((what,) + c(**kw) + (minimum,))

  robot, task = CASES[name][:2]
  if name in ('vase_crowd', 'wake_order'):
    need('sphere - pillar cc', a='robot', b='pillar', ga=0, branch='cc')
    for br in cb[:2]:
      need(f'arrow - pillar {br}', a='robot', b='pillar', ga=1, branch=br)
    for br in cb:
      need(f'sphere - vase {br}', a='robot', b='vase', ga=0, branch=br)
    need('arrow - vase bb, a vertex of the arrow only', a='robot', b='vase', ga=1, branch='bb', verts=lambda v: v[0] > 0 and v[1] == 0)
    need('arrow - vase bb, a vertex of the vase only', a='robot', b='vase', ga=1, branch='bb', verts=lambda v: v[0] == 0 and v[1] > 0)
    need('arrow - vase bb, vertices of both', a='robot', b='vase', ga=1, branch='bb', verts=lambda v: v[0] > 0 and v[1] > 0)
    for br in cb:
      need(f'vase - pillar {br}', a='vase', b='pillar', branch=br)
    need('vase - vase bb, a vertex of the first', a='vase', b='vase', branch='bb', verts=lambda v: v[0] > 0)
    need('vase - vase bb, a vertex of the second', a='vase', b='vase', branch='bb', verts=lambda v: v[1] > 0)
  elif name == 'buttons':
    need('sphere - button cc', a='robot', b='button', ga=0, branch='cc')
    need('arrow - button cb', a='robot', b='button', ga=1, branch=any_cb)
    need('vase - button cb', a='vase', b='button', branch=any_cb)
  elif task == 'push_box' and robot == 'point':
    for g in range(5):
      need(f'robot - box geom {g}', a='robot', b='object', gb=g)
      need(f'vase - box geom {g}', a='vase', b='object', gb=g)
    need('box - pillar', a='object', b='pillar')
  elif task == 'roll_rod':
    need('arrow - rod bb', a='robot', b='object', ga=1, branch='bb')
    need('sphere - rod cb', a='robot', b='object', ga=0, branch=any_cb)
    need('vase - rod bb', a='vase', b='object', branch='bb')
    need('rod - pillar', a='object', b='pillar')
  elif name == 'car_dribble_ball':   # every geom of the Car meets the ball's full radius (.14): only the Point's sphere sits .04 below its centre
    for g in range(8):
      need(f'car geom {g} - ball', 3, a='robot', b='object', ga=g)
    need('rear ball - ball cc', a='robot', b='object', ga=7, branch='cc')
  elif task == 'dribble_ball':
    need('sphere - ball cc', 10, a='robot', b='object', ga=0, branch='cc')
    need('arrow - ball cb', a='robot', b='object', ga=1, branch=any_cb)
    for br in cb:
      need(f'vase - ball {br}', a='vase', b='object', branch=br)
    need('ball - pillar cc', a='object', b='pillar', branch='cc')
  elif name == 'car_push_box':
    for g in range(8):
      need(f'car geom {g} - box', 3, a='robot', b='object', ga=g)
    need('car geoms 4..7 - box (bits >= 32 of the pair mask)', a='robot', b='object', ga=lambda g: g >= 4)
    need('rear ball cc', a='robot', ga=7, branch='cc')
    need('rear ball cb', a='robot', ga=7, branch=any_cb)
    for g in range(5):
      need(f'car - box geom {g}', a='robot', b='object', gb=g)
  return rows

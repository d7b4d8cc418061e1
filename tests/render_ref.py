"""NumPy float64 restatement of the ray-cast image: an INDEPENDENT per-pixel reference for k_render_rgb
(csrc/sag_render.hpp) and for the oracle's twin of it (oracle/sag_oracle_render.inc).

Written from DESIGN.md 3.5, the robot XMLs and the reference's constants (the table below cites each figure), not from
r_hit / sago_render: a geom here is a convex solid described by its surfaces, and a ray's hit is found by collecting the
analytic candidate roots of every surface (sphere and infinite-cylinder quadratics, cap and slab planes) and keeping the
smallest t > 1e-6 whose point lies on the solid and where the ray ENTERS (d.n < 0).  A camera inside a geom therefore sees
nothing of it.  Everything is vectorised over the rays of an image.

Compositing: the opaque surface is the nearest opaque geom, else the floor, else the sky; the translucent entries in front
of it are sorted by distance (equal distances keep geom order), and the nearest 12 are blended back to front.

Decided pixels: the float colour is evaluated at the pixel centre and at four offsets of +-1e-6 pixel in u and v.  A pixel
is DECIDED when the five colours agree within 1e-6 per channel, else EDGE-UNDECIDED (a hard decision - which surface,
which checker square - flips inside the pixel's centre neighbourhood).  The colour rule alone also gives up pixels where
nothing flips: at the silhouette of a sphere of a pixel's size (a lidar ring seen by a far camera) the shade falls by
more than one unit per pixel, about one pixel in a thousand of an overlay image.  So a pixel is decided as well when its
five evaluations took the SAME hard decisions (opaque geom and face, checker square, the ordered list of layers and their
faces): the colour is smooth there and is compared exactly, which only adds pixels to the exact comparison.
A channel is ROUNDING-AMBIGUOUS when x * 255 + 0.5 lies within 1e-6 of an integer (the 0.7 floor square lands on exactly
179.0): it may take either neighbour.
COINCIDENT opaque surfaces (within 1e-9 m: the knee sphere that a Doggo's red hip capsule and its blue or green ankle
capsule share, doggo.xml:23-26) are one surface with two colours; which geom a ray caster finds nearer there is rounding
noise of the body frames.  The reference states the earlier geom's colour, keeps the other as `alt`, and a pixel there
may show either, exactly.  check() is the assertion every comparison uses."""
import os

import numpy as np

# ---- the table: sizes and colours, each with its source in the reference (file:line) ---------------------------------
T_MIN = 1e-6
MAX_LAYERS = 12                                  # "the nearest 12"
MAX_GEOMS = 112                                  # "lane 0 builds <= 112 geoms"
SKY_TOP, SKY_BOTTOM = (0.527, 0.582, 0.906), (0.1, 0.1, 0.35)   # mujoco_bridge.py:91-92 skybox gradient rgb1 -> rgb2
FLOOR_HALF = 3.5                                 # 7 x 7 m floor
FLOOR_SQUARE = 0.35                              # mujoco_bridge.py:97-102: 2 x 2 checker texture, texrepeat 10 10 over 7 m
FLOOR_RGB = (0.7, 0.8)                           # mujoco_bridge.py:99 rgb1, rgb2
SHADE = (0.4, 0.6, 0.2)                          # .4 + .6 max(n_z, 0) + .2 max(-n.d, 0), clamped
HAZARD = dict(rgb=(0, 0, 1), alpha=0.25, half=1e-2, z=2e-2)   # consts.py:24-25, primitive_objects.py:94,98-99
VASE = dict(rgb=(0, 1, 1), alpha=1.0, sink=4e-5)              # consts.py:19-20, primitive_objects.py:46,49
PILLAR = dict(rgb=(.5, .5, 1), alpha=1.0, half=0.5, z=0.5)    # consts.py:32-33, primitive_objects.py:118-119
GOAL = dict(rgb=(0, 1, 0), alpha=0.25, r=0.3, half=0.15, z=0.16, alpha_unsupervised=0.1)
#   consts.py:36, primitive_objects.py:135,139-140 (size .3: tasks/go_to_goal.py GOAL_SIZE); Unsupervised: DESIGN.md 3.5
BUTTON = dict(r=0.1, rgb=(1, 105 / 255, 180 / 255), rgb_goal=(0, 1, 0))   # press_buttons.py:15-16,82-91, collect.py:35,45
BOX = dict(rgb=(1, 1, 0), alpha=0.25, half=0.2, col_half=0.1, col_at=0.2)   # push_box.py:12,14,33-34,40-65
ROD = dict(rgb=(1, 1, 1), r=0.08, half_len=0.3)              # roll_rod.py:11-12,28,34,37 (drawn as a box: DESIGN.md 3.5)
BALL = dict(rgb=(1, 1, 1), r=0.14)                           # dribble_ball.py:30,36 (SPHERE_RADIUS = BOX_SIZE = .14)
ROBOT_RGB = (1, 0, 0)                                        # point.xml:5, car.xml:5, doggo.xml:6
BODY_Z = 0.1                                                 # point.xml:13, car.xml:12
DOGGO_Z0 = 0.22                                              # doggo.xml:12
POINT = dict(r=0.1, arrow_at=0.1, arrow_half=0.05)           # point.xml:18-19
CAR_BOXES = [((0, 0, 0), (.1, .1, .05)), ((0, .15, 0), (.1, .01, .05)), ((0, .125, 0), (.01, .025, .03)),
             ((0, -.165, 0), (.05, .01, .05)), ((0, -.13, .04), (.05, .03, .01))]   # car.xml:16-20
CAR_WHEELS = [((-.155, .1, -.05), (-.105, .1, -.05)), ((.105, .1, -.05), (.155, .1, -.05))]   # car.xml:21-28 (body pos + fromto)
CAR_WHEEL_R = 0.05                                           # car.xml:5 default size
CAR_REAR = ((0, -.1, -.05), 0.05)                            # car.xml:29-31
# doggo.xml:15-72 in the order of the oracle's doggo_debug geom axes (tests/test_oracle_doggo.py pins them):
# torso front, aux_1, aux_4, hip_1, ankle_1, hip_4, ankle_4, torso rear, aux_2, aux_3, hip_2, ankle_2, hip_3, ankle_3
DOGGO_R = [.075, .032, .032, .032, .032, .032, .032, .075, .032, .032, .032, .032, .032, .032]   # doggo.xml:6,15,48
DOGGO_CAPSULE = [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]                                       # doggo.xml:6,15,48
DOGGO_RGB = [ROBOT_RGB] * 4 + [(0, 0, 1), ROBOT_RGB, (0, 0, 1)] + [ROBOT_RGB] * 4 + [(0, 1, 0), ROBOT_RGB, (0, 1, 0)]   # :26,40,58,72
# cameras: position, xyaxes, fovy (point.xml:14, car.xml:14 with MuJoCo's default fovy 45, doggo.xml:13)
VISION = [((0, 0, .15), (0, -1, 0), (.4, 0, 1), 90.0), ((0, .1, .2), (-1, 0, 0), (0, -.4, 1), 45.0),
          ((.125, 0, .2), (0, -1, 0), (.4, 0, 1), 100.0)]
FIXED_OFFSET = {1: 2.0, 2: 5.0, 3: 2.0}          # mujoco_bridge.py:128-129,143-150: (0, -off, off), zaxis 0 -1 1, fovy 45
RING = dict(r=0.025, at=0.15, z0=0.5, dz=0.06, bins=16)      # render.py:5,13,38,45
RING_COLS = (0, 32, 16)                          # safe_adaptation_gym.py:139,248-250: rings obstacles, goal, objects
COST = dict(r=0.25, rgb=(1, 0, 0), alpha=0.5)    # render.py:31-32, safe_adaptation_gym.py:255
TASK_COLLECT, TASK_PRESS, TASK_PRESS_SCARCE, TASK_UNSUPERVISED = 1, 8, 9, 13   # include/sag.h
F_ROBOT, F_HAZARD_SIZE, F_VASE_SIZE, F_PILLAR_SIZE, F_GOAL, F_BOX, F_HAZARDS, F_PILLARS, F_BUTTONS, F_VASES, F_EXT = (
    0, 24, 25, 26, 32, 41, 47, 65, 69, 81, 144)
I_TASK, I_NH, I_NV, I_NP, I_NB, I_BOX_KIND, I_GOAL_BUTTON, I_BTN_STATE, I_ACTIVE_MASK = 0, 1, 2, 3, 4, 5, 6, 7, 10
OFFSETS = ((0.0, 0.0), (1e-6, 0.0), (-1e-6, 0.0), (0.0, 1e-6), (0.0, -1e-6))
DECIDED_TOL = 1e-6
UNDECIDED_CAP = 1e-4
TIE = 1e-9       # opaque surfaces nearer to each other than this coincide
CHUNK = 1 << 15   # rays per pass (bounds the [layers, rays, 3] arrays of the compositing)


# ---- solids ------------------------------------------------------------------------------------------------------------
def _rotz(a):
  c, s = np.cos(a), np.sin(a)
  return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _quat_mat(q):
  w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class Geom:
  """A convex solid with colour.  hit(o, d) -> (t [M], n [M, 3], part [M]); t = inf where the ray does not enter it."""

  def __init__(self, name, rgb, alpha, centre):
    self.name, self.rgb, self.alpha, self.centre = name, np.asarray(rgb, np.float64), float(alpha), np.asarray(centre, np.float64)

  def hit(self, o, d):
    """The candidate roots are evaluated for the rays whose line has real roots with the geom's quadric at all (every ray for a
    box): arithmetic saved, no decision taken."""
    m = self.real_roots(o, d)
    best = [np.full(len(d), np.inf), np.zeros_like(d), np.zeros(len(d), int)]
    if m.any():
      t, n, part = self.roots(o, d[m])
      best[0][m], best[1][m], best[2][m] = t, n, part
    return best

  def real_roots(self, o, d):
    return np.ones(len(d), bool)


def _take(best, t, n, part, ok, d):
  """Candidate root t with normal n: kept where it is valid, in front, entering and nearer than what is held."""
  with np.errstate(invalid='ignore'):
    ok = ok & np.isfinite(t) & (t > T_MIN) & (np.einsum('mk,mk->m', n, d) < 0) & (t < best[0])
  best[0] = np.where(ok, t, best[0])
  best[1] = np.where(ok[:, None], n, best[1])
  best[2] = np.where(ok, part, best[2])


def _quadratic(a, b, c):
  """Both roots of a t^2 + 2 b t + c = 0 (nan where there is none)."""
  with np.errstate(invalid='ignore', divide='ignore'):
    s = np.sqrt(b * b - a * c)
    return (-b - s) / a, (-b + s) / a


class Sphere(Geom):

  def __init__(self, name, c, r, rgb, alpha):
    super().__init__(name, rgb, alpha, c)
    self.c, self.r = np.asarray(c, np.float64), float(r)

  def real_roots(self, o, d):
    oc = o - self.c
    return (d @ oc)**2 - (oc @ oc - self.r**2) > 0

  def roots(self, o, d):
    best = [np.full(len(d), np.inf), np.zeros_like(d), np.zeros(len(d), int)]
    oc = o - self.c
    for t in _quadratic(1.0, d @ oc, oc @ oc - self.r**2):
      n = (oc + np.nan_to_num(t)[:, None] * d) / self.r
      _take(best, t, n, 0, np.ones(len(d), bool), d)
    return best


class Rod(Geom):
  """Cylinder (flat caps) or capsule of radius r about the segment a -> e.  part: 0 side, 1 the end at a, 2 the end at e."""

  def __init__(self, name, a, e, r, capsule, rgb, alpha):
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    super().__init__(name, rgb, alpha, 0.5 * (a + e))
    self.a, self.e, self.r, self.capsule = a, e, float(r), bool(capsule)
    self.L = np.linalg.norm(e - a)
    self.u = (e - a) / self.L

  def real_roots(self, o, d):
    """Every point of the cylinder and of the capsule lies within r of the axis' line."""
    oa = o - self.a
    dperp, operp = d - (d @ self.u)[:, None] * self.u, oa - (oa @ self.u) * self.u
    a, b, c = np.einsum('mk,mk->m', dperp, dperp), dperp @ operp, operp @ operp - self.r**2
    return (b * b - a * c > 0) | (a == 0)

  def roots(self, o, d):
    M = len(d)
    best = [np.full(M, np.inf), np.zeros_like(d), np.zeros(M, int)]
    u, r, L = self.u, self.r, self.L
    oa = o - self.a
    du, ou = d @ u, oa @ u
    dperp, operp = d - du[:, None] * u, oa - ou * u
    with np.errstate(invalid='ignore', divide='ignore'):
      for t in _quadratic(np.einsum('mk,mk->m', dperp, dperp), dperp @ operp, operp @ operp - r * r):   # the side
        tt = np.nan_to_num(t)
        s = ou + tt * du
        _take(best, t, (operp + tt[:, None] * dperp) / r, 0, (s >= 0) & (s <= L), d)
      for part, s0, sign in ((1, 0.0, -1.0), (2, L, 1.0)):
        if self.capsule:     # the half of the end sphere beyond the segment's end
          centre = self.a + s0 * u
          oc = o - centre
          for t in _quadratic(1.0, d @ oc, oc @ oc - r * r):
            tt = np.nan_to_num(t)
            s = ou + tt * du
            _take(best, t, (oc + tt[:, None] * d) / r, part, sign * (s - s0) >= 0, d)
        else:                # the flat cap: the disc of the plane s = s0
          t = (s0 - ou) / du
          q = operp + np.nan_to_num(t)[:, None] * dperp
          _take(best, t, np.broadcast_to(sign * u, d.shape), part, np.einsum('mk,mk->m', q, q) <= r * r, d)
    return best


class Box(Geom):
  """Box of half extents h, rotated by yaw about z.  part: 1 + face index."""

  def __init__(self, name, c, half, yaw, rgb, alpha):
    super().__init__(name, rgb, alpha, c)
    self.c, self.h, self.A = np.asarray(c, np.float64), np.asarray(half, np.float64), _rotz(yaw)   # columns: the box's axes

  def real_roots(self, o, d):
    """Every point of the box lies within its half diagonal of the centre."""
    oc = o - self.c
    return (d @ oc)**2 - (oc @ oc - self.h @ self.h) > 0

  def roots(self, o, d):
    M = len(d)
    best = [np.full(M, np.inf), np.zeros_like(d), np.zeros(M, int)]
    lo, ld = (o - self.c) @ self.A, d @ self.A
    with np.errstate(invalid='ignore', divide='ignore'):
      for k in range(3):
        for sign in (-1.0, 1.0):
          t = (sign * self.h[k] - lo[k]) / ld[:, k]
          q = lo + np.nan_to_num(t)[:, None] * ld
          ok = np.ones(M, bool)
          for j in range(3):
            if j != k:
              ok &= np.abs(q[:, j]) <= self.h[j]
          _take(best, t, np.broadcast_to(sign * self.A[:, k], d.shape), 1 + 2 * k + (sign > 0), ok, d)
    return best


def upright_cylinder(name, x, y, z, r, half, rgb, alpha):
  return Rod(name, (x, y, z - half), (x, y, z + half), r, False, rgb, alpha)


# ---- scene and camera --------------------------------------------------------------------------------------------------
def body_frame(rf, robot):
  rf = np.asarray(rf, np.float64)
  if robot == 2:
    if not rf[F_EXT + 1:F_EXT + 5].any():   # include/sag.h: a zero quaternion means "upright at ROBOT yaw, z = 0.22" (doggo.xml:12)
      return _rotz(rf[F_ROBOT + 2]), np.array([rf[F_ROBOT], rf[F_ROBOT + 1], DOGGO_Z0])
    return _quat_mat(rf[F_EXT + 1:F_EXT + 5]), np.array([rf[F_ROBOT], rf[F_ROBOT + 1], rf[F_EXT]])
  return _rotz(rf[F_ROBOT + 2]), np.array([rf[F_ROBOT], rf[F_ROBOT + 1], BODY_Z])


def camera(robot, cam, R, p):
  """-> origin, X, Y, Z (the camera looks along -Z), tan(fovy / 2)"""
  if cam == 0:
    pos, x, y, fovy = VISION[robot]
    x = np.asarray(x, np.float64) / np.linalg.norm(x)
    y = np.asarray(y, np.float64) - np.dot(x, y) * x
    y /= np.linalg.norm(y)
    return p + R @ np.asarray(pos, np.float64), R @ x, R @ y, R @ np.cross(x, y), np.tan(np.radians(fovy) / 2)
  off = FIXED_OFFSET[cam]
  base = p if cam == 3 else np.zeros(3)
  z = np.array([0.0, -1.0, 1.0]) / np.sqrt(2.0)
  x = np.array([1.0, 0.0, 0.0])
  return base + np.array([0.0, -off, off]), x, np.cross(z, x), z, np.tan(np.radians(45.0) / 2)


def scene(rf, ri, robot, overlays=False, obs48=None, cost=0, doggo_axes=None):
  """The geoms of one record in model order.  doggo_axes: [14, 6] world end points of the Doggo's geoms."""
  rf, ri = np.asarray(rf, np.float64), np.asarray(ri)
  R, p = body_frame(rf, robot)
  task = int(ri[I_TASK])
  g = []
  for k in range(ri[I_NH]):
    x, y = rf[F_HAZARDS + 2 * k:F_HAZARDS + 2 * k + 2]
    g.append(upright_cylinder(f'hazard{k}', x, y, HAZARD['z'], rf[F_HAZARD_SIZE], HAZARD['half'], HAZARD['rgb'], HAZARD['alpha']))
  vs = rf[F_VASE_SIZE]
  for k in range(ri[I_NV]):
    x, y, yaw = rf[F_VASES + 6 * k:F_VASES + 6 * k + 3]
    g.append(Box(f'vase{k}', (x, y, vs - VASE['sink']), (vs, vs, vs), yaw, VASE['rgb'], VASE['alpha']))
  for k in range(ri[I_NP]):
    x, y = rf[F_PILLARS + 2 * k:F_PILLARS + 2 * k + 2]
    g.append(upright_cylinder(f'pillar{k}', x, y, PILLAR['z'], rf[F_PILLAR_SIZE], PILLAR['half'], PILLAR['rgb'], PILLAR['alpha']))
  if task not in (TASK_COLLECT, TASK_PRESS, TASK_PRESS_SCARCE):
    g.append(upright_cylinder('goal', rf[F_GOAL], rf[F_GOAL + 1], GOAL['z'], GOAL['r'], GOAL['half'], GOAL['rgb'],
                              GOAL['alpha_unsupervised'] if task == TASK_UNSUPERVISED else GOAL['alpha']))
  for b in range(ri[I_NB]):
    if task == TASK_COLLECT:
      green = bool(ri[I_ACTIVE_MASK] >> b & 1)
    else:
      green = ri[I_BTN_STATE] != 0 and b == ri[I_GOAL_BUTTON]
    x, y = rf[F_BUTTONS + 2 * b:F_BUTTONS + 2 * b + 2]
    g.append(Sphere(f'button{b}', (x, y, BUTTON['r']), BUTTON['r'], BUTTON['rgb_goal'] if green else BUTTON['rgb'], 1.0))
  bx, by, byaw = rf[F_BOX:F_BOX + 3]
  if ri[I_BOX_KIND] == 1:
    h, w, at = BOX['half'], BOX['col_half'], BOX['col_at']
    g.append(Box('box', (bx, by, h), (h, h, h), byaw, BOX['rgb'], BOX['alpha']))
    for k, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
      c = _rotz(byaw) @ np.array([sx * at, sy * at, 0.0]) + (bx, by, h)
      g.append(Box(f'col{k + 1}', c, (w, w, h), byaw, BOX['rgb'], BOX['alpha']))
  elif ri[I_BOX_KIND] == 2:
    g.append(Box('rod', (bx, by, ROD['r']), (ROD['r'], ROD['half_len'], ROD['r']), byaw, ROD['rgb'], 1.0))
  elif ri[I_BOX_KIND] == 3:
    g.append(Sphere('ball', (bx, by, BALL['r']), BALL['r'], BALL['rgb'], 1.0))
  at = lambda v: p + R @ np.asarray(v, np.float64)   # noqa: E731
  if robot == 0:
    g.append(Sphere('robot', p, POINT['r'], ROBOT_RGB, 1.0))
    g.append(Box('pointarrow', at((POINT['arrow_at'], 0, 0)), (POINT['arrow_half'],) * 3, rf[F_ROBOT + 2], ROBOT_RGB, 1.0))
  elif robot == 1:
    for k, (pos, half) in enumerate(CAR_BOXES):
      g.append(Box(f'car{k}', at(pos), half, rf[F_ROBOT + 2], ROBOT_RGB, 1.0))
    for k, (a, e) in enumerate(CAR_WHEELS):
      g.append(Rod(f'wheel{k}', at(a), at(e), CAR_WHEEL_R, False, ROBOT_RGB, 1.0))
    g.append(Sphere('rear', at(CAR_REAR[0]), CAR_REAR[1], ROBOT_RGB, 1.0))
  else:
    ax = np.asarray(doggo_axes, np.float64).reshape(14, 6)
    for k in range(14):
      g.append(Rod(f'doggo{k}', ax[k, :3], ax[k, 3:], DOGGO_R[k], DOGGO_CAPSULE[k], DOGGO_RGB[k], 1.0))
  if overlays:
    for ring, col0 in enumerate(RING_COLS):
      for j in range(RING['bins']):
        th = 2.0 * np.pi * (j + 0.5) / RING['bins']
        al = min(1.0, (0.0 if obs48 is None else float(obs48[col0 + j])) + 0.1)
        rgb = [0.0, 0.0, 0.0]
        rgb[ring] = al
        g.append(Sphere(f'ring{ring}_{j}', at((RING['at'] * np.cos(th), RING['at'] * np.sin(th), RING['z0'] + RING['dz'] * ring)),
                        RING['r'], rgb, al))
    if cost:
      g.append(Sphere('cost', p, COST['r'], COST['rgb'], COST['alpha']))
  return g, R, p


def _shade(rgb, n, d):
  s = SHADE[0] + SHADE[1] * np.maximum(n[:, 2], 0) + SHADE[2] * np.maximum(-np.einsum('mk,mk->m', n, d), 0)
  return np.minimum(s, 1.0)[:, None] * rgb


def _trace(geoms, o, d):
  """-> colour [M, 3], the colour with the other of two coincident opaque surfaces [M, 3] and where there is one [M], layers
  in front of the opaque surface [M], opaque geom index [M] (-1 floor, -2 sky), its part [M], [M] bool: some visible geom's
  centre lies behind the ray's origin, signature of the hard decisions taken [M]"""
  M = len(d)
  t_op, base, alt = np.full(M, np.inf), np.zeros((M, 3)), np.zeros((M, 3))
  surf, part, behind_op, tied = np.full(M, -2), np.zeros(M, int), np.zeros(M, bool), np.zeros(M, bool)
  hits = {}
  for k, gm in enumerate(geoms):
    t, n, pt = gm.hit(o, d)
    if not np.isfinite(t).any():
      continue
    if gm.alpha >= 1.0:
      # two opaque surfaces within TIE of each other coincide (the knee sphere that a Doggo's hip and ankle capsules share):
      # the earlier geom is the stated surface and the later one's colour the alternative
      with np.errstate(invalid='ignore'):
        nearer, tie = t < t_op - TIE, np.abs(t - t_op) <= TIE
      sh = _shade(gm.rgb, n, d)
      alt = np.where(tie[:, None], sh, alt)
      tied = np.where(nearer, False, tied | tie)
      t_op = np.where(nearer, t, t_op)
      base = np.where(nearer[:, None], sh, base)
      surf, part = np.where(nearer, k, surf), np.where(nearer, pt, part)
      behind_op = np.where(nearer, d @ (gm.centre - o) < 0, behind_op)
    else:
      hits[k] = (t, n, pt)
  # the floor: the plane z = 0 inside the 7 x 7 m square
  with np.errstate(divide='ignore', invalid='ignore'):
    tf = -o[2] / d[:, 2]
    fx, fy = o[0] + tf * d[:, 0], o[1] + tf * d[:, 1]
    on = (d[:, 2] < 0) & (tf > T_MIN) & (tf < t_op) & (np.abs(fx) <= FLOOR_HALF) & (np.abs(fy) <= FLOOR_HALF)
    odd = (np.floor((fx + FLOOR_HALF) / FLOOR_SQUARE) + np.floor((fy + FLOOR_HALF) / FLOOR_SQUARE)) % 2 == 1
  grey = np.where(odd, FLOOR_RGB[1], FLOOR_RGB[0])
  up = np.broadcast_to(np.array([0.0, 0.0, 1.0]), d.shape)
  base = np.where(on[:, None], _shade(grey[:, None] * np.ones(3), up, d), base)
  t_op, surf, part = np.where(on, tf, t_op), np.where(on, -1, surf), np.where(on, odd.astype(int), part)
  behind_op &= ~on
  tied &= ~on
  sky = surf == -2
  w = 0.5 * (d[:, 2] + 1.0)
  base = np.where(sky[:, None], np.asarray(SKY_BOTTOM) + (np.asarray(SKY_TOP) - SKY_BOTTOM) * w[:, None], base)
  alt = np.where(tied[:, None], alt, base)
  sig = ((surf + 2) * 16 + part).astype(np.uint64)
  nlay, behind = np.zeros(M, int), behind_op.copy()
  if hits:
    ks = sorted(hits)
    T = np.stack([np.where(hits[k][0] < t_op, hits[k][0], np.inf) for k in ks])          # [G, M]
    SC = np.stack([_shade(geoms[k].rgb, hits[k][1], d) for k in ks])                        # [G, M, 3]
    PT = np.stack([hits[k][2] for k in ks])
    AL = np.array([geoms[k].alpha for k in ks])
    BH = np.stack([d @ (geoms[k].centre - o) < 0 for k in ks])
    nlay = np.isfinite(T).sum(0)
    at = np.flatnonzero(nlay > 0)                                                          # the rays with a layer
    order = np.argsort(T[:, at], axis=0, kind='stable')                                    # equal distances keep geom order
    for j in range(min(MAX_LAYERS, len(ks)) - 1, -1, -1):
      gi = order[j]
      use = j < nlay[at]
      a = AL[gi][:, None]
      base[at] = np.where(use[:, None], a * SC[gi, at] + (1 - a) * base[at], base[at])
      alt[at] = np.where(use[:, None], a * SC[gi, at] + (1 - a) * alt[at], alt[at])
      behind[at] |= use & BH[gi, at]
      sig[at] = np.where(use, sig[at] * np.uint64(1000003) + (gi * 16 + PT[gi, at] + 1).astype(np.uint64), sig[at])
  return np.clip(base, 0.0, 1.0), np.clip(alt, 0.0, 1.0), tied, nlay, surf, part, behind, sig


class Image:
  """The reference's statement of one image.  colour [5, H, W, 3] floats at the five sample points (0 = the pixel centre),
  rgb [H, W, 3] the rounded centre colour, alt [H, W, 3] floats: the centre colour with the other of two coincident opaque
  surfaces (= colour[0] elsewhere) and tied [H, W] where there is one, decided [H, W], ambiguous [H, W, 3],
  layers / surf / part / behind [H, W] (at the centre), geoms, origin (the camera's)."""


def render(rf, ri, robot, cam, W, H, overlays=False, obs48=None, cost=0, doggo_axes=None):
  geoms, R, p = scene(rf, ri, robot, overlays, obs48, cost, doggo_axes)
  assert len(geoms) <= MAX_GEOMS
  o, X, Y, Z, th = camera(robot, cam, R, p)
  r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  ds = []
  for du, dv in OFFSETS:
    u = ((c + 0.5 + du) / (0.5 * W) - 1.0) * th * (W / H)
    v = (1.0 - (r + 0.5 + dv) / (0.5 * H)) * th
    d = u[..., None] * X + v[..., None] * Y - Z
    ds.append((d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3))
  rays = np.concatenate(ds)
  parts = [_trace(geoms, o, rays[k:k + CHUNK]) for k in range(0, len(rays), CHUNK)]
  col, alt, tied, nlay, surf, part, behind, sig = (np.concatenate(x) for x in zip(*parts))
  im = Image()
  im.geoms, im.W, im.H, im.origin = geoms, W, H, o
  im.colour = col.reshape(5, H, W, 3)
  im.rgb = _levels(im.colour[0]).astype(np.uint8)
  pick = lambda a: a.reshape((5, H, W) + a.shape[1:])[0]   # noqa: E731
  im.alt, im.tied = pick(alt), pick(tied)
  sig = sig.reshape(5, H, W)
  im.decided = (np.abs(im.colour - im.colour[:1]).max((0, 3)) <= DECIDED_TOL) | (sig == sig[:1]).all(0)
  im.layers, im.surf, im.part, im.behind = pick(nlay), pick(surf), pick(part), pick(behind)
  return im


def _levels(colour):
  return np.floor(colour * 255.0 + 0.5).astype(int)


def _matches(got, colour):
  """got [..., 3] int levels against float colours, up to the rounding rule: a channel whose x * 255 + .5 sits within 1e-6 of an
  integer k may be k - 1 or k."""
  y = colour * 255.0 + 0.5
  k = np.round(y)
  return ((got == np.floor(y)) | ((np.abs(y - k) <= 1e-6) & ((got == k) | (got == k - 1)))).all(-1)


def check(img, refs, what='', cap=True):
  """The assertion of every comparison: `img` [n, H, W, 3] uint8 against the reference Images of the same envs.
  -> (pixels, edge-undecided pixels, pixels on coincident surfaces that show the later geom)."""
  img = np.asarray(img)
  assert img.dtype == np.uint8 and img.shape == (len(refs), refs[0].H, refs[0].W, 3), (img.dtype, img.shape)
  got = img.astype(int)
  decided, tied = np.stack([r.decided for r in refs]), np.stack([r.tied for r in refs])
  first = _matches(got, np.stack([r.colour[0] for r in refs]))
  other = tied & _matches(got, np.stack([r.alt for r in refs]))
  bad = decided & ~first & ~other
  if bad.any():
    e, r, c = np.argwhere(bad)[0]
    g = refs[e]
    s = int(g.surf[r, c])
    raise AssertionError(f'{what}: {int(bad.sum())} DECIDED pixels differ; first: env {e} row {r} col {c}: image {got[e, r, c]}, '
                         f'reference {g.rgb[r, c]} (surface {g.geoms[s].name if s >= 0 else ("floor", "sky")[-1 - s]}, '
                         f'{int(g.layers[r, c])} layers)')
  five = np.stack([np.concatenate([_levels(r.colour), _levels(r.alt)[None]]) for r in refs])   # [n, 6, H, W, 3]
  near = (np.abs(five - got[:, None]) <= 1).all(-1).any(1)
  off = ~decided & ~near
  assert not off.any(), f'{what}: {int(off.sum())} edge-undecided pixels equal none of the five evaluations; first {np.argwhere(off)[0]}'
  und = int((~decided).sum())
  assert not cap or und <= UNDECIDED_CAP * decided.size, f'{what}: {und} of {decided.size} pixels are edge-undecided: change the scene'
  return decided.size, und, int((decided & ~first).sum())


def render_batch(oracle, rf, ri, robot, cam, W, H, overlays=False, obs=None, cost=None, envs=None):
  """Reference Images of the records (of the envs listed, or all).  The world end points of the Doggo's 14 geoms come from the
  oracle's doggo_debug, whose kinematics tests/test_oracle_doggo.py pins against doggo.xml."""
  out = []
  for k in (range(len(rf)) if envs is None else envs):
    ax = oracle.doggo_debug(oracle.env(rf[k], ri[k]))[2][48:] if robot == 2 else None
    out.append(render(rf[k], ri[k], robot, cam, W, H, overlays, None if obs is None else obs[k, :48], 0 if cost is None else int(cost[k]), ax))
  return out


LOG_DIR_ENV = 'SAG_RENDER_LOG_DIR'   # a directory: the counts are appended to render_pixel_counts.txt there (unset: printed only)


def differing_pixels(oracle, img, ora, rf, ri, robot, cam, W, H, overlays=False, obs=None, cost=None, what=''):
  """The pixels in which a device image `img` differs from the oracle's `ora` [n, H, W, 3]: each must be one that the reference
  leaves open - edge-undecided, or on coincident surfaces - and show one of the reference's candidates.  -> their number, which
  is also logged (the measured counts behind the tests' budgets: profiles/render_pixel_counts.txt)."""
  bad = (np.asarray(img) != np.asarray(ora)).any(-1)
  envs = np.flatnonzero(bad.any((1, 2)))
  edge = coincident = 0
  for k, ref in zip(envs, render_batch(oracle, rf, ri, robot, cam, W, H, overlays, obs, cost, envs)):
    closed = bad[k] & ref.decided & ~ref.tied
    assert not closed.any(), (f'{what}: env {k}: {int(closed.sum())} pixels differ from the oracle that the reference decides; first '
                              f'{np.argwhere(closed)[0]}: device {img[k][closed][0]}, oracle {ora[k][closed][0]}, reference {ref.rgb[closed][0]}')
    edge, coincident = edge + int((bad[k] & ~ref.decided).sum()), coincident + int((bad[k] & ref.decided & ref.tied).sum())
    check(img[k:k + 1], [ref], what, cap=False)   # (the cap on undecided pixels is for scenes made for it: tests/test_render_ref.py)
  line = (f'{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle ({edge} edge-undecided, {coincident} on coincident '
          f'surfaces){" (host build)" if os.environ.get("SAG_HOSTEMU") else ""}')
  print(line)
  if os.environ.get(LOG_DIR_ENV):
    try:
      os.makedirs(os.environ[LOG_DIR_ENV], exist_ok=True)
      with open(os.path.join(os.environ[LOG_DIR_ENV], 'render_pixel_counts.txt'), 'a') as f:
        f.write(line + '\n')
    except OSError:
      pass
  return int(bad.sum())

"""NumPy float64 statement of the depth and segmentation images, the judge of sag_render_aux(_device).

Geoms, camera and rays are render_ref's (scene, camera, Geom.hit, OFFSETS, T_MIN, the floor constants); nothing here is
taken from the kernel.  Per sample point of a pixel (the centre and the four offsets of render_ref.OFFSETS):
  the SURFACE is the geom with the smallest hit distance t over ALL geoms, whatever their alpha (a translucent hazard disc
  or goal cylinder is a surface; on an exact tie the earlier geom), else the floor (z = 0 inside the 7 x 7 m square), else
  the sky;
  DEPTH is the distance from the camera plane, t / sqrt(1 + u^2 + v^2) with the sample's own (u, v) - the ray
  u X + v Y - Z has that length, and its component along the viewing direction -Z is 1 -, rounded once to float32; the
  sky holds SAG_DEPTH_SKY;
  SEGMENTATION is (instance, class) of the surface, from the geom's NAME (enum sag_seg_class); the sky is (-1, -1).
A pixel is DECIDED when its five samples meet the same surface, and TIED when a second GEOM lies within render_ref.TIE of
the nearest one at the centre (the coplanar tops of the PushBox box and its columns, a Doggo's knee sphere): either geom
may be stated there.  The floor takes no part in a tie.  check_*() are the assertions every comparison uses.

The Doggo's camera: render_ref.scene() takes the Doggo's geoms from the oracle's doggo_debug, which builds the body frame
from the record's quaternion AS STORED (float32: its norm is 1 only to 3e-8), but returns the frame of the NORMALISED
quaternion for the camera - two frames 3e-8 apart, which no colour shows and a depth of one float32 step does (12 steps at
.25 m).  Here the camera rides on the frame the geoms ride on: render_ref.camera() is given the rotation of the stored
quaternion (stored_frame), which for a unit quaternion is the same matrix."""
import re

import numpy as np

import render_ref as rr

DEPTH_SKY = np.float32(50.0)   # include/sag.h SAG_DEPTH_SKY: MuJoCo's default zfar, taken as metres
FLOOR, HAZARD, VASE, PILLAR, GOAL, BUTTON, OBJECT, ROBOT, LIDAR, COST = range(10)   # include/sag.h enum sag_seg_class
SKY = -1
CAR_ROBOT = {'wheel0': 5, 'wheel1': 6, 'rear': 7}


def seg_of_name(name):
  """(instance, class) of a geom of render_ref.scene()."""
  m = re.fullmatch(r'([a-z]+?)(\d*)(?:_(\d+))?', name)
  stem, k = m.group(1), int(m.group(2)) if m.group(2) else 0
  if stem in ('hazard', 'vase', 'pillar', 'button'):
    return k, {'hazard': HAZARD, 'vase': VASE, 'pillar': PILLAR, 'button': BUTTON}[stem]
  if name == 'goal':
    return 0, GOAL
  if name in ('box', 'rod', 'ball'):
    return 0, OBJECT
  if stem == 'col':
    return k, OBJECT                       # col1 .. col4 in build order
  if name == 'robot':
    return 0, ROBOT                        # the Point's sphere
  if name == 'pointarrow':
    return 1, ROBOT
  if stem == 'car':
    return k, ROBOT                        # the five boxes
  if name in CAR_ROBOT:
    return CAR_ROBOT[name], ROBOT
  if stem == 'doggo':
    return k, ROBOT                        # geom-table order
  if stem == 'ring':
    return k * 16 + int(m.group(3)), LIDAR
  if name == 'cost':
    return 0, COST
  raise KeyError(name)


def stored_frame(rf, robot, R):
  """The Doggo's body rotation from its quaternion as the record stores it (w^2 + x^2 - y^2 - z^2 on the diagonal: |q|^2 times
  a rotation), else R."""
  q = np.asarray(rf, np.float64)[rr.F_EXT + 1:rr.F_EXT + 5]
  if robot != 2 or not q.any():
    return R
  w, x, y, z = q
  return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


class AuxImage:
  """surf [5, H, W]: index of the surface's geom per sample (G = the floor, G + 1 = the sky, G = len(geoms)); depth [5, H, W]
  float64 (the sky: DEPTH_SKY); near [G, H, W] bool: the geoms within TIE of the nearest at the centre; tied, decided [H, W];
  seg_of [G + 2, 2] int: (instance, class) per surface index; seg [H, W, 2] int32 and depth32 [H, W] float32: the centre's."""


def trace(geoms, o, d):
  """-> surface index [M] (len(geoms): floor, len(geoms) + 1: sky), its t [M] (inf: sky), T [G, M] the geoms' own t"""
  G, M = len(geoms), len(d)
  T = np.full((G, M), np.inf)
  for k, gm in enumerate(geoms):
    T[k] = gm.hit(o, d)[0]
  if G:
    surf, t = np.argmin(T, 0), T.min(0)     # argmin: the first of equal minima = the earlier geom
    surf = np.where(np.isfinite(t), surf, G + 1)
  else:
    surf, t = np.full(M, G + 1), np.full(M, np.inf)
  with np.errstate(divide='ignore', invalid='ignore'):
    tf = -o[2] / d[:, 2]
    fx, fy = o[0] + tf * d[:, 0], o[1] + tf * d[:, 1]
    on = (d[:, 2] < 0) & (tf > rr.T_MIN) & (tf < t) & (np.abs(fx) <= rr.FLOOR_HALF) & (np.abs(fy) <= rr.FLOOR_HALF)
  return np.where(on, G, surf), np.where(on, tf, t), T


def render(rf, ri, robot, cam, W, H, overlays=False, obs48=None, cost=0, doggo_axes=None):
  geoms, R, p = rr.scene(rf, ri, robot, overlays, obs48, cost, doggo_axes)
  assert len(geoms) <= rr.MAX_GEOMS
  G = len(geoms)
  o, X, Y, Z, th = rr.camera(robot, cam, stored_frame(rf, robot, R), p)
  X, Y, Z = (a / np.linalg.norm(a) for a in (X, Y, Z))   # (the pixel's (u, v) are coordinates on unit axes)
  r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  im = AuxImage()
  im.geoms, im.W, im.H, im.origin = geoms, W, H, o
  im.surf, im.depth = np.zeros((5, H, W), int), np.zeros((5, H, W))
  for s, (du, dv) in enumerate(rr.OFFSETS):
    u = ((c + 0.5 + du) / (0.5 * W) - 1.0) * th * (W / H)
    v = (1.0 - (r + 0.5 + dv) / (0.5 * H)) * th
    d = u[..., None] * X + v[..., None] * Y - Z
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    surf, t, T = trace(geoms, o, d)
    with np.errstate(invalid='ignore'):
      depth = np.where(np.isfinite(t), t / np.sqrt(1.0 + u * u + v * v).reshape(-1), float(DEPTH_SKY))
    im.surf[s], im.depth[s] = surf.reshape(H, W), depth.reshape(H, W)
    if s == 0:
      with np.errstate(invalid='ignore'):
        near = (T <= T.min(0) + rr.TIE) & np.isfinite(T) & (surf < G) if G else np.zeros((0, H * W), bool)
      im.near = near.reshape(G, H, W)
      im.near_depth = np.where(near, T / np.sqrt(1.0 + u * u + v * v).reshape(-1), np.inf).reshape(G, H, W)
  im.tied = im.near.sum(0) > 1
  im.decided = (im.surf == im.surf[:1]).all(0)
  im.seg_of = np.array([seg_of_name(g.name) for g in geoms] + [(0, FLOOR), (SKY, SKY)], int).reshape(G + 2, 2)
  im.seg = im.seg_of[im.surf[0]].astype(np.int32)
  im.depth32 = im.depth[0].astype(np.float32)
  return im


def render_batch(oracle, rf, ri, robot, cam, W, H, overlays=False, obs=None, cost=None):
  """Reference images of the records; the Doggo's geom end points come from the oracle's doggo_debug, as render_ref.render_batch."""
  out = []
  for k in range(len(rf)):
    ax = oracle.doggo_debug(oracle.env(rf[k], ri[k]))[2][48:] if robot == 2 else None
    out.append(render(rf[k], ri[k], robot, cam, W, H, overlays, None if obs is None else obs[k, :48], 0 if cost is None else int(cost[k]), ax))
  return out


def _ulps(a, b):
  """Distance in float32 steps between two arrays of finite positive float32."""
  return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def _cap(refs, what):
  decided = np.stack([r.decided for r in refs])
  und = int((~decided).sum())
  assert und <= rr.UNDECIDED_CAP * decided.size, f'{what}: {und} of {decided.size} pixels are undecided: change the scene'
  return decided, und


def check_seg(img, refs, what='', cap=True):
  """img [n, H, W, 2] int32 (instance, class).  Decided, untied pixels: equal.  Tied: either tied geom.  Undecided: one of the
  five samples'.  -> (pixels, undecided, tied pixels)"""
  img = np.asarray(img)
  assert img.dtype == np.int32 and img.shape == (len(refs), refs[0].H, refs[0].W, 2), (img.dtype, img.shape)
  decided, und = _cap(refs, what) if cap else (np.stack([r.decided for r in refs]), 0)
  tied = np.stack([r.tied for r in refs])
  first = (img == np.stack([r.seg for r in refs])).all(-1)
  other = np.zeros_like(first)
  five = np.zeros_like(first)
  for e, r in enumerate(refs):
    for k in np.flatnonzero(r.near.any((1, 2))):
      other[e] |= r.near[k] & r.tied & (img[e] == r.seg_of[k]).all(-1)
    for s in range(5):
      five[e] |= (img[e] == r.seg_of[r.surf[s]]).all(-1)
  bad = decided & ~first & ~(tied & other)
  if bad.any():
    e, r, c = np.argwhere(bad)[0]
    raise AssertionError(f'{what}: {int(bad.sum())} DECIDED pixels differ; first: env {e} row {r} col {c}: image (instance, class) '
                         f'{img[e, r, c]}, reference {refs[e].seg[r, c]}')
  off = ~decided & ~five & ~(tied & other)
  assert not off.any(), f'{what}: {int(off.sum())} undecided pixels equal none of the five samples; first {np.argwhere(off)[0]}'
  return decided.size, int((~decided).sum()), int(tied.sum())


def check_depth(img, refs, what='', cap=True):
  """img [n, H, W] float32.  Decided, untied pixels: within 1 float32 step of the reference's rounded depth (both sides round
  one float64 once; the step covers a value on a rounding boundary); the sky exactly.  Tied: within a step of either tied
  geom's.  Undecided: within the span of the five samples' depths (and the rounding step) of one of them."""
  img = np.asarray(img)
  assert img.dtype == np.float32 and img.shape == (len(refs), refs[0].H, refs[0].W), (img.dtype, img.shape)
  assert np.isfinite(img).all() and (img > 0).all(), f'{what}: a depth that is not finite and positive'
  decided, und = _cap(refs, what) if cap else (np.stack([r.decided for r in refs]), 0)
  tied = np.stack([r.tied for r in refs])
  ref32 = np.stack([r.depth32 for r in refs])
  sky = np.stack([r.surf[0] == len(r.geoms) + 1 for r in refs])
  first = np.where(sky, img == DEPTH_SKY, _ulps(img, ref32) <= 1)
  other = np.zeros_like(first)
  five = np.zeros_like(first)
  for e, r in enumerate(refs):
    for k in np.flatnonzero(r.near.any((1, 2))):
      m = r.near[k] & r.tied
      other[e] |= m & (_ulps(img[e], np.where(m, r.near_depth[k], 1.0).astype(np.float32)) <= 1)
    span = r.depth.max(0) - r.depth.min(0)
    for s in range(5):
      d32 = r.depth[s].astype(np.float32)
      five[e] |= np.abs(img[e].astype(np.float64) - d32) <= span + np.spacing(d32)
  bad = decided & ~first & ~(tied & other)
  if bad.any():
    e, r, c = np.argwhere(bad)[0]
    raise AssertionError(f'{what}: {int(bad.sum())} DECIDED pixels differ by more than one float32 step; first: env {e} row {r} col {c}: '
                         f'image {img[e, r, c]!r}, reference {ref32[e, r, c]!r} ({refs[e].depth[0, r, c]!r})')
  off = ~decided & ~five & ~(tied & other)
  assert not off.any(), f'{what}: {int(off.sum())} undecided pixels lie outside the span of the five samples; first {np.argwhere(off)[0]}'
  return decided.size, int((~decided).sum()), int(tied.sum())

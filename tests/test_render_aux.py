"""Depth and segmentation images of the device ray caster (sag_render_aux, sag_render_aux_device; csrc/sag_render.hpp
k_render_rows<OUT> / k_render_list<OUT> with r_trace_nearest) against the NumPy statement tests/render_aux_ref.py, which takes its geoms, camera
and rays from render_ref.  The acceptance rule is render_aux_ref.check_seg / check_depth: at decided, untied pixels class and
instance equal and depth within one float32 step; at tied pixels either tied geom; at undecided pixels one of the five
samples; at most render_ref.UNDECIDED_CAP of a case's pixels undecided.  The cases are ten of test_render_ref.CASES."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import render_aux_ref as ra
import render_ref as rr
import test_render_ref as trr
from oracle_lib import F_HAZARD_SIZE, F_HAZARDS, F_PILLAR_SIZE, F_PILLARS, F_VASE_SIZE, F_VASES, Oracle
from test_render_ref import CAM, CASES, RID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SEG = 1, 2           # include/sag.h enum sag_render_output
ERR_ARG = -1                # include/sag.h SAG_ERR_ARG
SENTINEL = 0xA5
AUX_CASES = ['size 7x5 N=3', 'size 9x8 N=3', 'size 130x50 N=3', 'size 1x1 N=1', 'more than 12 layers, track',
             'camera inside a bounding sphere: the goal cylinder and the cost sphere', 'box kind box',
             'collect with three active masks', 'doggo tipped, joints at their range ends, vision', 'fullest scene']
ITEM = {DEPTH: 4, SEG: 8}   # bytes per pixel = the alignment sag_render_aux_device asks of d_out
DTYPE = {DEPTH: np.float32, SEG: np.int32}


@pytest.fixture(scope='module')
def oracle():
  return Oracle()


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


_REFS = {}


def _references(oracle, robot, camera, W, H, overlays, rf, ri, obs, cost):
  """Reference images, computed once per (records, overlay inputs) and never changed."""
  rid, cam = RID[robot], CAM[camera]
  key = (rid, cam, W, H, overlays, rf.tobytes(), ri.tobytes(), obs[:, :48].tobytes() if overlays else b'', cost.tobytes() if overlays else b'')
  if key not in _REFS:
    _REFS[key] = ra.render_batch(oracle, rf, ri, rid, cam, W, H, overlays, obs, cost)
  return _REFS[key]


def _shape(output, n, H, W):
  return (n, H, W) if output == DEPTH else (n, H, W, 2)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference's own known answers, and the cap on undecided pixels for the chosen cases
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_empty_floor_fixedfar():
  """fixedfar at (0, -5, 5) looks down its -Z = (0, 1, -1) / sqrt 2 at the origin: the centre of a 1 x 1 image is the floor at
  distance 5 sqrt 2 along the axis (u = v = 0: depth = t).  The floor ends at y = 3.5: rows above it are sky."""
  rf, ri = trr._record('point', 'go_to_goal', xy=trr.FAR)
  im = ra.render(rf.astype(np.float32), ri, 0, CAM['fixedfar'], 1, 1)
  assert im.decided.all() and (im.seg[0, 0] == (0, ra.FLOOR)).all()
  np.testing.assert_allclose(im.depth[0, 0, 0], 5 * np.sqrt(2), rtol=1e-15)
  im = ra.render(rf.astype(np.float32), ri, 0, CAM['fixedfar'], 9, 9)
  # pixel (row r, col 4): u = 0, v = (1 - (r + .5) / 4.5) tan 22.5; the ray (0, v + 1, v - 1) / sqrt 2 meets z = 0 at
  # t' = 5 sqrt 2 / (1 - v) of the unnormalised ray = the depth, at y = -5 + 5 (1 + v) / (1 - v): on the floor while y <= 3.5
  v = (1 - (np.arange(9) + 0.5) / 4.5) * np.tan(np.radians(22.5))
  y = -5 + 5 * (1 + v) / (1 - v)
  on = np.abs(y) <= 3.5
  assert on.sum() >= 3 and (~on).sum() >= 2 and not on[0], 'sky above the floor\'s edge'
  np.testing.assert_allclose(im.depth[0, on, 4], 5 * np.sqrt(2) / (1 - v[on]), rtol=1e-14)
  assert (im.seg[on, 4] == (0, ra.FLOOR)).all()
  assert (im.depth32[~on, 4] == ra.DEPTH_SKY).all() and ra.DEPTH_SKY == np.float32(50.0) and (im.seg[~on, 4] == (-1, -1)).all()


def test_reference_vase_in_front_of_pillar_and_hazard_over_floor():
  """The Point at the origin looks along +x (its camera .15 above the body at z .1, tilted up): a vase at x = 1 hides the
  lower part of a pillar at x = 2; a hazard disc (translucent) in front of the floor is HAZARD, not FLOOR."""
  rf, ri = trr._record('point', 'go_to_goal', nh=2, nv=2, np_=1)
  rf[F_VASES:F_VASES + 3] = [2.8, 2.8, 0.0]
  rf[F_VASES + 6:F_VASES + 9] = [1.0, 0.0, 0.0]        # vase 1, half size rf[F_VASE_SIZE] (.1): x in [.9, 1.1], z up to .2
  rf[F_PILLARS:F_PILLARS + 2] = [2.0, 0.0]
  rf[F_HAZARDS:F_HAZARDS + 4] = [2.8, -2.8, 0.0, 0.0]  # hazard 1 under the robot
  rf[F_HAZARD_SIZE] = 0.9
  im = ra.render(rf.astype(np.float32), ri, 0, CAM['vision'], 65, 65)
  seg, col = im.seg, 32                                 # (the centre column: u = 0)
  rows_v = np.flatnonzero((seg[:, col] == (1, ra.VASE)).all(-1))
  rows_p = np.flatnonzero((seg[:, col] == (0, ra.PILLAR)).all(-1))
  assert len(rows_v) >= 2 and len(rows_p) >= 5 and rows_p.max() < rows_v.min(), 'the pillar shows above the vase only'
  # column 32 has u = 0: the unnormalised ray is v Y - Z, and its parameter at a plane is the depth itself
  o, (X, Y, Z) = im.origin, rr.camera(0, 0, *rr.body_frame(rf, 0))[1:4]
  assert o[2] == pytest.approx(0.25)
  ray = lambda r: (1.0 - (r + 0.5) / 32.5) * np.tan(np.radians(45.0)) * Y - Z   # noqa: E731
  vs = float(np.float32(rf[F_VASE_SIZE]))
  for r in rows_v:     # the vase (a convex box): the later of the entries into its slabs x >= 1 - vs and z <= 2 vs - 4e-5
    front, top = (1.0 - vs - o[0]) / ray(r)[0], (2 * vs - 4e-5 - o[2]) / ray(r)[2] if ray(r)[2] < 0 else -np.inf
    np.testing.assert_allclose(im.depth[0, r, col], max(front, top), rtol=1e-12)
  assert any((1.0 - vs - o[0]) / ray(r)[0] == pytest.approx(im.depth[0, r, col], rel=1e-12) for r in rows_v), 'the near face is in view'
  for r in rows_p:     # the pillar (radius rf[F_PILLAR_SIZE]) at x = 2, met head-on in the plane y = 0
    np.testing.assert_allclose(im.depth[0, r, col], (2.0 - float(np.float32(rf[F_PILLAR_SIZE])) - o[0]) / ray(r)[0], rtol=1e-12)
  # looking down in front of the robot: the disc (top at z = .03), not the floor, and .03 nearer than the floor would be
  rows_h = np.flatnonzero((seg[:, col] == (1, ra.HAZARD)).all(-1))
  assert len(rows_h) >= 5 and not (seg[..., 1] == ra.FLOOR)[rows_h, col].any()
  for r in rows_h:     # the disc's top, the plane z = .03
    np.testing.assert_allclose(im.depth[0, r, col], (0.03 - o[2]) / ray(r)[2], rtol=1e-12)


def test_seg_of_name_covers_every_class():
  got = {ra.seg_of_name(n) for n in ('hazard3', 'vase9', 'pillar1', 'goal', 'button5', 'box', 'col4', 'rod', 'ball', 'robot', 'pointarrow',
                                     'car4', 'wheel0', 'wheel1', 'rear', 'doggo13', 'ring2_15', 'cost')}
  assert got == {(3, ra.HAZARD), (9, ra.VASE), (1, ra.PILLAR), (0, ra.GOAL), (5, ra.BUTTON), (0, ra.OBJECT), (4, ra.OBJECT), (0, ra.ROBOT),
                 (1, ra.ROBOT), (4, ra.ROBOT), (5, ra.ROBOT), (6, ra.ROBOT), (7, ra.ROBOT), (13, ra.ROBOT), (47, ra.LIDAR), (0, ra.COST)}


def _expect(name, refs):
  """What a case is for under the new rule, asserted from the reference."""
  cls = np.stack([r.seg[..., 1] for r in refs])
  inst = np.stack([r.seg[..., 0] for r in refs])
  if name.startswith('more than 12 layers'):
    # the nearest surface is translucent where RGB's opaque one is something else
    assert ((cls == ra.HAZARD) | (cls == ra.COST) | (cls == ra.OBJECT)).sum() >= 100
  if name == 'box kind box':
    assert sum(int(r.tied.sum()) for r in refs) > 0, 'no tied pixel: the box\'s top and its columns\' are coplanar'
    assert len(np.unique(inst[cls == ra.OBJECT])) >= 3, 'column instances'
  if name == 'fullest scene':
    assert set(range(10)) <= set(np.unique(cls)), f'every class in view: {np.unique(cls)}'


@pytest.mark.parametrize('name', AUX_CASES)
def test_cases_meet_the_cap_under_the_aux_rule(oracle, name):
  """No GPU: the chosen scenes leave at most UNDECIDED_CAP of their pixels undecided under this file's rule (five samples on
  one surface), and the reference passes its own check."""
  robot, camera, W, H, overlays, records, _ = CASES[name]
  rf, ri = records()
  obs, cost = trr._oracle_overlay_inputs(oracle, robot, rf, ri)
  refs = _references(oracle, robot, camera, W, H, overlays, rf, ri, obs, cost)
  _expect(name, refs)
  total, und, tied = ra.check_seg(np.stack([r.seg for r in refs]), refs, name)
  ra.check_depth(np.stack([r.depth32 for r in refs]), refs, name)
  print(f'{name}: {total} pixels, {und} undecided, {tied} tied')


def test_aux_cases_on_the_host_build():
  """This file's GPU cases on the UNSANITIZED host build of the library's own sources (tests/hostemu), selected with
  SAG_LIB + SAG_HOSTEMU as test_hostemu_variants.test_front_end_api_on_the_emulated_device does: every case passes, none is
  skipped.  A checker of the device source without a GPU, never a product path."""
  sys.path.insert(0, os.path.join(ROOT, 'tests', 'hostemu'))
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.fail('no clang for the host build of the kernel')
  lib = hb.build('clang', False, False, [], False, False, 'var_base')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-q', '-p', 'no:cacheprovider'],
                     env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
  tail = r.stdout[-3000:] + r.stderr[-3000:]
  assert r.returncode == 0, tail
  summary = r.stdout.strip().splitlines()[-1]
  passed = re.search(r'(\d+) passed', summary)
  assert passed and int(passed.group(1)) == len(AUX_CASES) + 5 and 'skipped' not in summary and 'failed' not in summary, summary


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _context(nat, robot, rf, ri):
  n = len(rf)
  ctx = nat.Context(robot, n, seed=5)
  ctx.set_layout(rf, ri)
  out = ctx.step(np.zeros((n, ctx.info['nu']), np.float32), nstep=0)
  return ctx, out[0], out[2]


class _Overlay:
  """Device copies of the observation and cost rows that the overlays show."""

  def __init__(self, ctx, overlays, obs, cost):
    self.ctx, self.d_obs, self.d_cost = ctx, None, None
    if overlays:
      self.d_obs, self.d_cost = ctx.dev_alloc(obs.nbytes), ctx.dev_alloc(ctx.n_envs)
      ctx.dev_upload(self.d_obs, np.ascontiguousarray(obs, np.float32))
      ctx.dev_upload(self.d_cost, np.ascontiguousarray(cost, np.uint8))

  def free(self):
    for p in (self.d_obs, self.d_cost):
      if p is not None:
        self.ctx.dev_free(p)


def _aux_device(ctx, output, cam, W, H, overlays, ov, mask=None, rc_want=0, shift=None):
  """sag_render_aux_device into a caller's buffer at a byte offset of one pixel (4 B depth, 8 B segmentation), sentinel bytes
  before and after.  -> the rows as raw bytes [n, H * W * item] and as values."""
  n, item = ctx.n_envs, ITEM[output]
  lead = item if shift is None else shift
  size, tail = n * H * W * item, 8
  d_out = ctx.dev_alloc(lead + size + tail)
  ctx.dev_upload(d_out, np.full(lead + size + tail, SENTINEL, np.uint8))
  d_mask = None
  if mask is not None:
    d_mask = ctx.dev_alloc(n)
    ctx.dev_upload(d_mask, np.ascontiguousarray(mask, np.uint8))
  rc = ctx.lib.sag_render_aux_device(ctx.h, output, cam, W, H, 1 if overlays else 0, ov.d_obs, ov.d_cost, d_mask, C.c_void_p(d_out.value + lead))
  ctx.wait()
  buf = ctx.dev_download(d_out, (lead + size + tail,), np.uint8)
  ctx.dev_free(d_out)
  if d_mask is not None:
    ctx.dev_free(d_mask)
  assert rc == rc_want, (rc, ctx.lib.sag_last_error(ctx.h))
  assert (buf[:lead] == SENTINEL).all() and (buf[lead + size:] == SENTINEL).all(), 'bytes outside the image were written'
  raw = buf[lead:lead + size].reshape(n, -1)
  if rc_want:
    assert (raw == SENTINEL).all(), 'a refused call wrote to the buffer'
    return raw, None
  return raw, np.frombuffer(raw.tobytes(), DTYPE[output]).reshape(_shape(output, n, H, W)) if raw.size else None


@pytest.mark.gpu
@pytest.mark.parametrize('name', AUX_CASES)
def test_device_aux_images_equal_the_reference(nat, oracle, name):
  robot, camera, W, H, overlays, records, _ = CASES[name]
  rf, ri = records()
  ctx, obs, cost = _context(nat, robot, rf, ri)
  rf2, ri2 = ctx.get_state()
  same = np.r_[0:2, 24:27, 32:34, 41:44, 47:141, 144:149, 153:166]   # poses and sizes: the step of no substeps moved nothing
  np.testing.assert_array_equal(rf2[:, same], rf[:, same], err_msg='the scene is no longer the case')
  np.testing.assert_array_equal(ri2[:, np.r_[0:8, 10]], ri[:, np.r_[0:8, 10]], err_msg='the scene is no longer the case')
  ov = _Overlay(ctx, overlays, obs, cost)
  depth = _aux_device(ctx, DEPTH, CAM[camera], W, H, overlays, ov)[1]
  seg = _aux_device(ctx, SEG, CAM[camera], W, H, overlays, ov)[1]
  ov.free()
  ctx.close()
  refs = _references(oracle, robot, camera, W, H, overlays, rf2, ri2, obs, cost)
  _expect(name, refs)
  total, und, tied = ra.check_seg(seg, refs, name)
  ra.check_depth(depth, refs, name)
  sky = seg[..., 1] == ra.SKY
  assert (depth[sky] == ra.DEPTH_SKY).all() and (depth[~sky] < ra.DEPTH_SKY).all() and (seg[sky] == -1).all()
  print(f'{name}: {total} pixels, {und} undecided, {tied} tied')


def _three(nat):
  """3 Point / push_box envs at 7 x 5 with overlays ('size 7x5 N=3')."""
  robot, camera, W, H, overlays, records, _ = CASES['size 7x5 N=3']
  rf, ri = records()
  ctx, obs, cost = _context(nat, robot, rf, ri)
  return ctx, CAM[camera], W, H, obs, cost


@pytest.mark.gpu
def test_masked_form_writes_the_rows_of_its_mask_only(nat):
  ctx, cam, W, H, obs, cost = _three(nat)
  ov = _Overlay(ctx, True, obs, cost)
  for output in (DEPTH, SEG):
    whole = _aux_device(ctx, output, cam, W, H, True, ov)[0]
    assert not (whole == SENTINEL).all(1).any()
    some = _aux_device(ctx, output, cam, W, H, True, ov, mask=[1, 0, 1])[0]
    assert (some[1] == SENTINEL).all(), 'the row of an env outside the mask was written'
    np.testing.assert_array_equal(some[[0, 2]], whole[[0, 2]])
    np.testing.assert_array_equal(_aux_device(ctx, output, cam, W, H, True, ov, mask=[7, 255, 1])[0], whole)   # any non-zero byte
    assert (_aux_device(ctx, output, cam, W, H, True, ov, mask=[0, 0, 0])[0] == SENTINEL).all(), 'an all-zero mask wrote something'
  ov.free()
  ctx.close()


def _aux_host(ctx, output, cam, W, H, overlays, ids, n=None, rows=None, null_out=False):
  """sag_render_aux into a host buffer of sentinel bytes -> (rc, raw rows [rows, H * W * item])"""
  ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
  n = (0 if ids is None else len(ids)) if n is None else n
  rows = (ctx.n_envs if ids is None else len(ids)) if rows is None else rows
  out = np.full((rows, H * W * ITEM.get(output, 8)), SENTINEL, np.uint8)
  rc = ctx.lib.sag_render_aux(ctx.h, output, cam, W, H, 1 if overlays else 0, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)),
                              n, None if null_out else out.ctypes.data_as(C.c_void_p))
  return rc, out


@pytest.mark.gpu
def test_listed_form_and_refused_arguments(nat):
  ctx, cam, W, H, obs, cost = _three(nat)   # (the step of _context left obs / cost in the context's own buffers: the overlays' rows)
  ov = _Overlay(ctx, True, obs, cost)
  for output in (DEPTH, SEG):
    whole = _aux_device(ctx, output, cam, W, H, True, ov)[0]
    rc, rows = _aux_host(ctx, output, cam, W, H, True, [2, 0, 2])
    assert rc == 0
    np.testing.assert_array_equal(rows, whole[[2, 0, 2]])
    rc, rows = _aux_host(ctx, output, cam, W, H, True, None, n=-7)      # NULL list: every env, n is ignored
    assert rc == 0
    np.testing.assert_array_equal(rows, whole)
    rc, rows = _aux_host(ctx, output, cam, W, H, True, [1], n=0, rows=1)
    assert rc == 0 and (rows == SENTINEL).all(), 'n == 0 wrote something'
    assert _aux_host(ctx, output, cam, W, H, True, [1], n=0, null_out=True)[0] == 0
    for what, kw in (('n < 0', dict(ids=[0, 1], n=-1)), ('an index of n_envs', dict(ids=[0, 3])), ('a negative index', dict(ids=[-1, 0])),
                     ('a bad camera', dict(ids=[0, 1], cam=4)), ('a negative camera', dict(ids=[0, 1], cam=-1)),
                     ('width 0', dict(ids=[0, 1], W=0)), ('height 4097', dict(ids=[0, 1], H=4097)),
                     ('NULL out', dict(ids=[0, 1], null_out=True)), ('NULL out, every env', dict(ids=None, null_out=True))):
      a = dict(cam=cam, W=W, H=H, n=None, null_out=False)
      a.update(kw)
      # (the host buffer is sized for the good image: a refused call reads none of it)
      out = np.full(3 * H * W * ITEM[output], SENTINEL, np.uint8)
      ids = None if a['ids'] is None else np.array(a['ids'], np.int32)
      rc = ctx.lib.sag_render_aux(ctx.h, output, a['cam'], a['W'], a['H'], 1, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                  (0 if ids is None else len(ids)) if a['n'] is None else a['n'], None if a['null_out'] else out.ctypes.data_as(C.c_void_p))
      assert rc == ERR_ARG, f'{what}: {rc}'
      assert (out == SENTINEL).all(), f'{what}: the buffer was written'
    # the device form: a misaligned d_out, a bad camera, a bad size
    _aux_device(ctx, output, cam, W, H, True, ov, rc_want=ERR_ARG, shift=ITEM[output] // 2)
    _aux_device(ctx, output, 4, W, H, True, ov, rc_want=ERR_ARG)
    _aux_device(ctx, output, cam, W, 0, True, ov, rc_want=ERR_ARG)
    _aux_device(ctx, output, cam, W, H, True, ov, mask=[1, 1, 1], rc_want=ERR_ARG, shift=ITEM[output] // 2)
    assert ctx.lib.sag_render_aux_device(ctx.h, output, cam, W, H, 1, None, None, None, None) == ERR_ARG
  for output in (0, 3, -1):   # an unknown output (0 would be the RGB image: it has its own entry points)
    rc, rows = _aux_host(ctx, output, cam, W, H, True, [0, 1])
    assert rc == ERR_ARG and (rows == SENTINEL).all()
    d = ctx.dev_alloc(3 * W * H * 8)
    ctx.dev_upload(d, np.full(3 * W * H * 8, SENTINEL, np.uint8))
    assert ctx.lib.sag_render_aux_device(ctx.h, output, cam, W, H, 1, None, None, None, d) == ERR_ARG
    ctx.wait()
    assert (ctx.dev_download(d, (3 * W * H * 8,), np.uint8) == SENTINEL).all()
    ctx.dev_free(d)
  ov.free()
  ctx.close()


@pytest.mark.gpu
def test_rgb_render_is_the_same_before_and_after_aux_calls(nat):
  """Staging bookkeeping (the aux calls grow and reuse the RGB staging buffer at other sizes) and no state written."""
  ctx, cam, W, H, obs, cost = _three(nat)
  rf0, ri0 = ctx.get_state()
  before = ctx.render(camera=cam, width=40, height=30, overlays=True)
  some_before = ctx.render(camera=cam, width=40, height=30, overlays=True, envs=[2, 1])
  assert _aux_host(ctx, DEPTH, cam, 7, 5, True, [1])[0] == 0           # smaller than the RGB staging
  assert _aux_host(ctx, SEG, cam, 130, 50, True, None)[0] == 0         # larger: the staging grows
  assert _aux_host(ctx, DEPTH, cam, 64, 64, False, [0, 0, 1, 2])[0] == 0
  assert _aux_host(ctx, SEG, 0, 1, 1, False, [2])[0] == 0
  np.testing.assert_array_equal(ctx.render(camera=cam, width=40, height=30, overlays=True, envs=[2, 1]), some_before)
  np.testing.assert_array_equal(ctx.render(camera=cam, width=40, height=30, overlays=True), before)
  assert _aux_host(ctx, SEG, cam, 200, 100, True, None)[0] == 0
  np.testing.assert_array_equal(ctx.render(camera=cam, width=40, height=30, overlays=True), before)
  rf1, ri1 = ctx.get_state()
  np.testing.assert_array_equal(rf1, rf0)
  np.testing.assert_array_equal(ri1, ri0)
  ctx.close()


def _make(devices, **kw):
  """make(); on the host emulation of the device sources, which runs one kernel at a time, the shards take turns
  (test_reset_loop._serial)."""
  import safe_adaptation_gym_amd as sag
  env = sag.make('point', 'go_to_goal', seed=3, n_envs=3, devices=devices, **kw)
  if os.environ.get('SAG_HOSTEMU') and env._pool is not None:
    env._pool.shutdown()
    env._pool = None
  return env


@pytest.mark.gpu
@pytest.mark.parametrize('devices', [[0], [0, 0]])
def test_env_api_depth_and_segmentation(nat, devices):
  kw = dict(camera_id='track', height=9, width=13)
  env = _make(devices, render_options=kw)
  env.reset()
  env.step(np.zeros((3, 2), np.float32))
  rgb = env.render()
  assert rgb.shape == (3, 9, 13, 3) and rgb.dtype == np.uint8
  depth, seg = env.render(depth=True), env.render(segmentation=True)
  assert depth.shape == (3, 9, 13) and depth.dtype == np.float32 and np.isfinite(depth).all() and (depth > 0).all()
  assert seg.shape == (3, 9, 13, 2) and seg.dtype == np.int32
  assert ((seg[..., 1] == ra.ROBOT).any((1, 2))).all(), 'the tracking camera sees the robot'
  assert ((seg[..., 1] == ra.SKY) == (depth == ra.DEPTH_SKY)).all()
  np.testing.assert_array_equal(env.render(depth=True, envs=[2, 0]), depth[[2, 0]])
  np.testing.assert_array_equal(env.render(segmentation=True, envs=[2, 0]), seg[[2, 0]])
  assert env.render(depth=True, envs=[]).shape == (0, 9, 13) and env.render(segmentation=True, envs=[]).shape == (0, 9, 13, 2)
  with pytest.raises(ValueError):
    env.render(depth=True, segmentation=True)
  np.testing.assert_array_equal(env.render(depth=False, segmentation=False), rgb)
  np.testing.assert_array_equal(env.render(), rgb)
  env.close()
  # the render_options route
  for opt, want in ((dict(depth=True), depth), (dict(segmentation=True), seg)):
    env = _make(devices, render_options=dict(kw, **opt))
    env.reset()
    env.step(np.zeros((3, 2), np.float32))
    np.testing.assert_array_equal(env.render(), want)
    np.testing.assert_array_equal(env.render(envs=[1]), want[[1]])
    env.close()
  env = _make(devices, render_options=dict(kw, depth=True, segmentation=True))
  env.reset()
  with pytest.raises(ValueError):
    env.render()
  env.close()

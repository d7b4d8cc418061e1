"""Rendering a chosen subset of the envs (k_render_rows<OUT> / k_render_list<OUT> of csrc/sag_render.hpp through the host's
render_launch / render_to_host: sag_render_rows_device and sag_render_envs) and what the env builds on it: rgb_observation
inside the stream-ordered episode loop (time_limit, auto_reset, reset(mask, sync=False)), the masked render of the synchronous
reset(mask), and render(envs=...).

Every comparison is byte-exact against the whole-batch render of the same state, which tests/test_render_ref.py ties to the
independent per-pixel reference.  Every GPU test here also runs on the host build of the device sources (tests/hostemu) at
the reduced sizes given first."""
import numpy as np
import pytest

import reset_sampler_ref as R
from test_device_reset import KEY
from test_reset_loop import (CASES, EPISODE0, HOSTEMU, _actions, _DevMask, _m_bytes, _m_first, _m_last, _m_ones,
                             _m_zeros, _make, _make_env, _np, _same, _tid)

MASKS = {'zeros': _m_zeros, 'ones': _m_ones, 'null': None, 'first': _m_first, 'last': _m_last, 'bytes': _m_bytes}


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


def _sentinel(shape):
  """A byte pattern no render produces over a whole row (period 251: it does not repeat with the image's rows)."""
  return (np.arange(int(np.prod(shape)), dtype=np.int64) % 251 + 3).astype(np.uint8).reshape(shape)


def _stepped(nat, case, n, steps=3):
  """A mixed-task context of `case` (tests/test_reset_loop.CASES) a few host-buffer steps into its episode: the context's own
  observation and cost buffers hold what the overlays show.  -> context, last observation, last cost flags."""
  robot, pick, config = CASES[case]
  tids, doe = pick(n)
  c, descs, doe = _make(nat, robot, tids, n, doe, config=config)
  rc, st, b = c.reset_device(True, episode0=EPISODE0)
  assert rc == 0 and not st.any()
  rng = np.random.RandomState(7)
  for t in range(steps):
    out = c.step(_actions(robot, *c.get_state(), rng, 3 if robot == 'doggo' else t))
  return c, out[0], out[2]


# ---------------------------------------------------------------------------------------------------------------------
# 1. masked render, C level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['point-mixed', 'car-mixed', 'doggo-mixed'])
def test_masked_render_writes_the_rows_of_its_mask_only(nat, case):
  """sag_render_rows_device into a buffer pre-filled with a sentinel pattern: the rows of the mask equal render_rgb()'s,
  every other byte is still the sentinel - for the masks of test_async_reset.SCHEDULE (all zero, all ones, NULL, first env,
  last env, bytes other than 0 / 1), at a batch that is no multiple of 64 and at one env; then the human view (fixedfar,
  overlays, 21 x 13) against render() of the whole batch."""
  doggo = case.startswith('doggo')
  big = (24 if HOSTEMU else 70) if doggo else (67 if HOSTEMU else 203)
  assert big % 64 and big % 256
  for n in (big, 1):
    c, obs, cost = _stepped(nat, case, n)
    if n == big:
      i = c.get_state()[1]
      seen = {'buttons': (i[:, R.I_NB] > 0).any(), 'boxes': (i[:, R.I_BOX_KIND] > 0).any(), 'hazards': (i[:, R.I_NH] > 0).any()}
      assert all(seen.values()), seen   # buttons, boxes and both translucent kinds (hazards; goals and boxes) are in the scenes
    ref = c.render_rgb()
    dm = _DevMask(c)
    img = c.dev_alloc(ref.nbytes)
    fill = _sentinel(ref.shape)
    rng = np.random.RandomState(3)
    for name, kind in MASKS.items():
      m8 = np.ones(n, np.uint8) if kind is None else kind(n, rng, None)
      c.dev_upload(img, fill)
      c.render_rows_device(None if kind is None else dm(m8), img)
      c.wait()
      want = fill.copy()
      want[m8 != 0] = ref[m8 != 0]
      np.testing.assert_array_equal(c.dev_download(img, ref.shape, np.uint8), want, err_msg=f'{case}, {n} envs, mask {name}')
    c.dev_free(img)
    # the human view: another camera, the overlays of the env's own observation / cost rows, a size that is no multiple of the 8 x 8 tile
    W, H = 21, 13
    whole = c.render('fixedfar', W, H, overlays=True)
    plain = c.render('fixedfar', W, H, overlays=False)
    if n == big:
      assert (whole != plain).any(axis=(1, 2, 3)).sum() > 1, 'the overlays are visible (at 21 x 13 a ring sphere can fall between the rays)'
    d_obs, d_cost, img = c.dev_alloc(obs.nbytes), c.dev_alloc(n), c.dev_alloc(whole.nbytes)
    c.dev_upload(d_obs, obs); c.dev_upload(d_cost, cost.astype(np.uint8))
    fill = _sentinel(whole.shape)
    m8 = _m_bytes(n, rng, None) if n == big else np.ones(1, np.uint8)
    c.dev_upload(img, fill)
    c.render_rows_device(dm(m8), img, camera='fixedfar', width=W, height=H, overlays=True, d_obs=d_obs, d_cost=d_cost)
    c.wait()
    want = fill.copy()
    want[m8 != 0] = whole[m8 != 0]
    np.testing.assert_array_equal(c.dev_download(img, whole.shape, np.uint8), want, err_msg=f'{case}, {n} envs: human view')
    for p in (d_obs, d_cost, img):
      c.dev_free(p)
    dm.free(); c.close()


@pytest.mark.gpu
def test_rgb_entry_points_refuse_bad_arguments_and_agree(nat):
  """The C level of the four colour entry points on the 3-env scene of test_render_aux._three (7 x 5, overlays).  A bad
  camera, a bad size, a NULL out or a listed index outside [0, n_envs) returns SAG_ERR_ARG and leaves a sentinel-filled buffer
  as it was; sag_render_envs with n == 0 returns SAG_OK and writes nothing, with and without null pointers.  Then
  sag_render_device, sag_render_rows_device with a NULL and with an all-ones mask, sag_render and sag_render_envs([0, 1, 2])
  give byte-equal rows."""
  import ctypes as C
  from test_render_aux import ERR_ARG, SENTINEL, _Overlay, _three
  ctx, cam, W, H, obs, cost = _three(nat)   # (the step of _context left obs / cost in the context's own buffers: the host forms' overlays)
  lib, h, n, size = ctx.lib, ctx.h, ctx.n_envs, ctx.n_envs * H * W * 3
  assert n == 3
  ov = _Overlay(ctx, True, obs, cost)
  d_out, d_ones = ctx.dev_alloc(size), ctx.dev_alloc(n)
  ctx.dev_upload(d_ones, np.ones(n, np.uint8))
  u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))     # noqa: E731
  i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))    # noqa: E731

  def host(ids, cam=cam, W=W, H=H, n_=None, null_out=False, null_ids=False):
    """sag_render (ids None) or sag_render_envs into a host buffer of sentinel bytes sized for the good image"""
    out = np.full(size, SENTINEL, np.uint8)
    o = None if null_out else u8(out)
    if ids is None:
      return lib.sag_render(h, cam, W, H, 1, o), out
    ids = np.array(ids, np.int32)
    return lib.sag_render_envs(h, cam, W, H, 1, None if null_ids else i32(ids), len(ids) if n_ is None else n_, o), out

  def device(mask, cam=cam, W=W, H=H, null_out=False):
    """sag_render_device (mask 'none') or sag_render_rows_device (mask None: NULL) into a device buffer of sentinel bytes"""
    ctx.dev_upload(d_out, np.full(size, SENTINEL, np.uint8))
    o = None if null_out else d_out
    if mask == 'none':
      rc = lib.sag_render_device(h, cam, W, H, 1, ov.d_obs, ov.d_cost, o)
    else:
      rc = lib.sag_render_rows_device(h, cam, W, H, 1, ov.d_obs, ov.d_cost, mask, o)
    ctx.wait()
    return rc, ctx.dev_download(d_out, (size,), np.uint8)

  bad = (('camera 4', dict(cam=4)), ('camera -1', dict(cam=-1)), ('width 0', dict(W=0)), ('height 4097', dict(H=4097)),
         ('NULL out', dict(null_out=True)))
  for what, kw in bad:
    for name, call in (('sag_render', lambda: host(None, **kw)), ('sag_render_envs', lambda: host([0, 1, 2], **kw)),
                       ('sag_render_device', lambda: device('none', **kw)), ('sag_render_rows_device', lambda: device(d_ones, **kw)),
                       ('sag_render_rows_device, NULL mask', lambda: device(None, **kw))):
      rc, buf = call()
      assert rc == ERR_ARG, f'{name}, {what}: {rc}'
      assert (buf == SENTINEL).all(), f'{name}, {what}: the buffer was written'
  for what, kw in (('an index of n_envs', dict(ids=[0, n])), ('an index of -1', dict(ids=[-1, 0])), ('n < 0', dict(ids=[0, 1], n_=-1)),
                   ('a NULL list', dict(ids=[0, 1], null_ids=True))):
    rc, buf = host(**kw)
    assert rc == ERR_ARG, f'sag_render_envs, {what}: {rc}'
    assert (buf == SENTINEL).all(), f'sag_render_envs, {what}: the buffer was written'
  # an empty list is not an error, whatever the pointers
  rc, buf = host([1], n_=0)
  assert rc == 0 and (buf == SENTINEL).all(), 'n == 0 wrote something'
  assert host([1], n_=0, null_out=True)[0] == 0 and host([1], n_=0, null_out=True, null_ids=True)[0] == 0
  # the five ways to the whole batch
  rc, whole = device('none')
  assert rc == 0 and not (whole.reshape(n, -1) == SENTINEL).all(1).any()
  for name, got in (('sag_render_rows_device, NULL mask', device(None)), ('sag_render_rows_device, all ones', device(d_ones)),
                    ('sag_render', host(None)), ('sag_render_envs', host([0, 1, 2]))):
    assert got[0] == 0, name
    np.testing.assert_array_equal(got[1], whole, err_msg=name)
  np.testing.assert_array_equal(whole.reshape(n, H, W, 3), ctx.render(cam, W, H, overlays=True))
  for p in (d_out, d_ones):
    ctx.dev_free(p)
  ov.free()
  ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. listed render
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['point-mixed', 'doggo-mixed'])
def test_listed_render_equals_rows_of_the_whole_batch(nat, case):
  """Context.render(envs=...): row j is row envs[j] of the whole-batch image, at 64 x 64 `vision` and at 21 x 13 `track` with
  the overlays (which must follow the env, not the workgroup), for an empty list, one index, the reversed range, duplicates
  and a random subset; an index out of range raises and leaves the context usable; whole-batch renders between listed ones
  are right (the staging buffer is grown by either form and its recorded size must stay true)."""
  doggo = case.startswith('doggo')
  n = (24 if HOSTEMU else 70) if doggo else (67 if HOSTEMU else 203)
  c, obs, cost = _stepped(nat, case, n)
  rng = np.random.RandomState(5)
  lists = {'empty': [], 'one': [n - 1], 'reversed': list(range(n))[::-1], 'duplicates': [3, 0, 3, n - 1, 3, 0],
           'subset': rng.choice(n, n // 3, replace=False).tolist()}
  views = [('track', 21, 13, True), ('vision', 64, 64, False)]
  # the first call of the context is a listed one (a staging buffer for one small image), then the whole batch grows it
  first = c.render('track', 21, 13, overlays=True, envs=[n - 1])
  for cam, W, H, ov in views:
    whole = c.render(cam, W, H, overlays=ov)
    if (cam, W, H) == ('track', 21, 13):
      np.testing.assert_array_equal(first[0], whole[n - 1])
      assert (whole != c.render(cam, W, H, overlays=False)).any(axis=(1, 2, 3)).sum() > 1, 'the overlays are visible'
    for name, ids in lists.items():
      got = c.render(cam, W, H, overlays=ov, envs=ids)
      assert got.shape == (len(ids), H, W, 3) and got.dtype == np.uint8
      np.testing.assert_array_equal(got, whole[np.asarray(ids, np.int64)], err_msg=f'{case} {cam} {W} x {H}: list {name}')
    for bad in ([n], [-1], [0, n - 1, n], [2**32 + 1], np.array([-2**32], np.int64)):   # (the last two would wrap into range)
      with pytest.raises(nat.SagError):
        c.render(cam, W, H, overlays=ov, envs=bad)
    for bad in ([0.0, 1.0], [[0, 1]], np.zeros(n, bool)):
      with pytest.raises(ValueError):
        c.render(cam, W, H, overlays=ov, envs=bad)
    np.testing.assert_array_equal(c.render(cam, W, H, overlays=ov), whole, err_msg='the whole batch after listed renders')
  np.testing.assert_array_equal(c.render_rgb(), whole)
  c.close()


@pytest.mark.gpu
def test_listed_render_of_one_env_of_a_large_batch(nat):
  """4096 envs, envs=[17] at the human view's default 256 x 256: one image comes back (the whole batch would be 805 MB) and
  it is the image of a one-env context holding env 17's state."""
  if HOSTEMU:
    pytest.skip('4096 envs at 256 x 256: a GPU-sized case (the host build runs the same call at 67 envs)')
  n = 4096
  c, descs, doe = _make(nat, 'point', [_tid('go_to_goal'), _tid('push_box')], n)
  assert c.reset_device(True, episode0=EPISODE0)[0] == 0
  got = c.render('fixedfar', 256, 256, overlays=False, envs=[17])
  assert got.shape == (1, 256, 256, 3)
  f, i = c.get_state()
  one = nat.Context('point', 1, seed=KEY)
  one.set_state(f[17:18], i[17:18])
  np.testing.assert_array_equal(got, one.render('fixedfar', 256, 256, overlays=False))
  np.testing.assert_array_equal(c.render('vision', 16, 16, overlays=False, envs=[n - 1, 17])[1],
                                one.render('vision', 16, 16, overlays=False)[0])
  one.close(); c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. env.render(envs=...)
# ---------------------------------------------------------------------------------------------------------------------
def _check_env_render(devices):
  n = 40 if HOSTEMU else 130
  kw = {} if devices is None else {'devices': devices}
  env = _make_env('point', 'push_box', n_envs=n, seed=19, **kw)
  env.reset()
  env.step(np.random.RandomState(0).uniform(-1, 1, (n, 2)).astype(np.float32))
  opt = dict(camera_id='track', width=21, height=13)
  whole = env.render(**opt)
  assert whole.shape == (n, 13, 21, 3)
  rng = np.random.RandomState(1)
  for ids in ([n - 1, 0, n // 2, 0, n - 1], list(range(n))[::-1], rng.choice(n, n // 4, replace=False), np.array([n // 3], np.uint8),
              [], np.zeros(0, np.int32), list(range(env._ranges[-1][0], n))):
    got = env.render(envs=ids, **opt)
    assert got.shape == (len(ids), 13, 21, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, whole[np.asarray(ids, np.int64)])
  before = env.get_state()
  for bad in (np.zeros(n, bool), np.array([1., 2.]), np.array([[1, 2]]), [0, -1], [n], np.int64(3), [2**40]):
    with pytest.raises(ValueError):
      env.render(envs=bad, **opt)
  _same(before, env.get_state(), 'state after refused lists')
  np.testing.assert_array_equal(env.render(**opt), whole)
  env.close()


@pytest.mark.gpu
@pytest.mark.parametrize('devices', [None, [0, 0, 0]], ids=['1 shard', 'devices=[0, 0, 0]'])
def test_env_render_of_listed_envs(nat, devices):
  """env.render(envs=...): global indices in the caller's order, across shards (some lists leave a shard without an entry),
  and the lists it refuses - bool, float, 2-D, 0-D, negative, too large - each with ValueError."""
  _check_env_render(devices)


@pytest.mark.gpu
def test_env_render_of_listed_envs_on_two_devices(nat):
  if nat.device_count() < 2:
    pytest.skip('needs 2 GPUs (the 8-GPU node of the driver runs it)')
  _check_env_render([0, 1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6. stream-ordered resets with images
# ---------------------------------------------------------------------------------------------------------------------
def _twin_images(env):
  """The whole-batch render of the twin's state (it returns vector observations; its contexts render all the same)."""
  env.wait()
  return np.concatenate([c.render_rgb() for c in env._ctx])


def _goals_onto_robots(nat, envs, rng):
  f, i = envs[0].get_state()
  g = rng.rand(len(f)) < 0.25
  f[g, nat.F_GOAL:nat.F_GOAL + 2] = f[g, nat.F_ROBOT:nat.F_ROBOT + 2]
  for e in envs:
    e.set_state(f, i)


def _act(robot, n, rng, t):
  if robot == 'doggo':
    a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
    return a * 0 if t < 3 else a
  return rng.uniform(-1, 1, (n, 2)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('robot,task,devices', [('point', 'go_to_goal', None), ('doggo', 'haul_box', None), ('point', 'press_buttons', [0, 0, 0])],
                         ids=['point', 'doggo', 'point, devices=[0, 0, 0]'])
def test_auto_reset_rollout_with_images_equals_the_vector_twin(nat, robot, task, devices):
  """A = make(rgb_observation, device_buffers, device_reset) with episode_loop(time_limit=5, auto_reset=True); B =
  make(device_buffers, device_reset, time_limit=5, auto_reset=True), no images;
  same seeds, same actions.  After every step the states are equal, A's image view is the whole-batch render of B's state
  (for an ended env: the first image of its new episode), and done / terminated / episode / reward / cost are equal.  A
  masked reset(sync=False) after step 2 staggers the episodes, so steps end some envs and not others."""
  n = (24 if HOSTEMU else 70) if robot == 'doggo' else (67 if HOSTEMU else 203)
  T, limit = (8 if HOSTEMU else 12), 5
  kw = dict(n_envs=n, seed=37, device_buffers=True, **({} if devices is None else {'devices': devices}))
  A, B = _make_env(robot, task, rgb_observation=True, **kw), _make_env(robot, task, time_limit=limit, auto_reset=True, **kw)
  A.episode_loop(time_limit=limit, auto_reset=True)
  img = A.reset(); B.reset()
  np.testing.assert_array_equal(_np(img), _twin_images(B))
  rng = np.random.RandomState(2)
  m30 = rng.rand(n) < 0.3
  mixed = ended_total = 0
  for t in range(T):
    if t in (4, 7):
      _goals_onto_robots(nat, (A, B), rng)
    act = _act(robot, n, rng, t)
    a, b = A.step(act, sync=False), B.step(act, sync=False)
    A.wait(); B.wait()
    _same(A.get_state(), B.get_state(), f'step {t}: state')
    assert _np(a[0]).shape == (n, 64, 64, 3) and _np(a[0]).dtype == np.uint8
    np.testing.assert_array_equal(_np(a[0]), _twin_images(B), err_msg=f'step {t}: images')
    _same([_np(a[1]), _np(a[2]), _np(a[3]['terminated']), _np(a[3]['episode']), _np(a[3]['cost']), _np(a[3]['goal_met'])],
          [_np(b[1]), _np(b[2]), _np(b[3]['terminated']), _np(b[3]['episode']), _np(b[3]['cost']), _np(b[3]['goal_met'])], f'step {t}')
    ended = _np(a[2]) != 0
    ended_total += int(ended.sum())
    mixed += int(ended.any() and not ended.all())
    if t == 2:
      kept = _np(a[0]).copy()
      img = A.reset(mask=m30, sync=False); B.reset(mask=m30, sync=False)
      A.wait()
      _same(A.get_state(), B.get_state(), 'state after reset(mask, sync=False)')
      got, want = _np(img), _twin_images(B)
      np.testing.assert_array_equal(got, want)
      np.testing.assert_array_equal(got[~m30], kept[~m30])
      assert (got[m30] != kept[m30]).any(axis=(1, 2, 3)).all()
  assert mixed >= 2 and ended_total >= n, (mixed, ended_total)   # steps that ended some envs and not others; every env ended once
  assert A.reset_counts() == B.reset_counts() and A.reset_counts()[1] == 0
  A.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize('robot,task', [('point', 'go_to_goal'), ('doggo', 'go_to_goal')])
def test_time_limit_then_masked_async_reset_with_images(nat, robot, task):
  """time_limit without auto_reset: the image a step returns is the final observation (the twin's render before its reset);
  reset(mask=done, sync=False) then renders the rows of the mask alone - they equal the twin's render of the new state, the
  others are byte for byte what the step returned.  Masks: a host bool array, the `done` device view; mask=None renders
  every env; and the synchronous reset(mask) returns the same bytes as a whole-batch render."""
  n = (24 if HOSTEMU else 70) if robot == 'doggo' else (67 if HOSTEMU else 131)
  kw = dict(n_envs=n, seed=41, device_buffers=True)
  A, B = _make_env(robot, task, rgb_observation=True, **kw), _make_env(robot, task, time_limit=4, **kw)
  A.episode_loop(time_limit=4)
  A.reset(); B.reset()
  rng = np.random.RandomState(6)
  host = rng.rand(n) < 0.4
  resets = {1: 'host bool', 3: 'done view', 5: 'done view', 6: 'none', 7: 'sync host'}
  partial = 0
  for t in range(8):
    act = _act(robot, n, rng, 3)
    a, b = A.step(act), B.step(act)
    final = _np(a[0]).copy()
    np.testing.assert_array_equal(final, _twin_images(B), err_msg=f'step {t}: the final observation')
    np.testing.assert_array_equal(_np(a[2]), _np(b[2]), err_msg=f'step {t}: done')
    kind = resets.get(t)
    if kind is None:
      continue
    done = _np(a[2]) != 0
    if kind == 'host bool':
      m, img = host, A.reset(mask=host, sync=False)
      B.reset(mask=host, sync=False)
    elif kind == 'done view':
      m, img = done, A.reset(mask=a[2], sync=False)
      B.reset(mask=b[2], sync=False)
      assert done.any() and not done.all(), f'step {t}: the time limit should end some envs'
      partial += 1
    elif kind == 'none':
      m, img = np.ones(n, bool), A.reset(sync=False)
      B.reset(sync=False)
    else:
      m, img = ~host, A.reset(mask=~host)
      B.reset(mask=~host)
    A.wait()
    _same(A.get_state(), B.get_state(), f'{kind} reset after step {t}: state')
    got, want = _np(img), _twin_images(B)
    np.testing.assert_array_equal(got[m], want[m], err_msg=f'{kind} reset after step {t}: images of the reset envs')
    np.testing.assert_array_equal(got[~m], final[~m], err_msg=f'{kind} reset after step {t}: rows outside the mask')
    np.testing.assert_array_equal(got, want, err_msg=f'{kind} reset after step {t}: an image is a function of the state')
    assert (got[m] != final[m]).any(axis=(1, 2, 3)).all()
  assert partial == 2
  # the state changed behind the image buffer (set_state): the next masked reset renders every row, not the mask's alone
  f, i = A.get_state()
  f[:, nat.F_ROBOT:nat.F_ROBOT + 2] *= 0.5
  A.set_state(f, i); B.set_state(f, i)
  img = A.reset(mask=host, sync=False); B.reset(mask=host, sync=False)
  A.wait()
  got = _np(img)
  np.testing.assert_array_equal(got, _twin_images(B), err_msg='reset(mask, sync=False) after set_state')
  assert (got[~host] != final[~host]).any(axis=(1, 2, 3)).all(), 'rows outside the mask show the state that was set'
  A.close(); B.close()


@pytest.mark.gpu
def test_sampling_failure_keeps_the_image_row(nat):
  """The impossible descriptor of test_async_reset.test_async_reset_commits_env_by_env under an image env: in
  reset(mask, sync=False) the env that cannot be laid out keeps its state, so the masked render reproduces its row - the
  row is unchanged by value - and reset_counts() reports it."""
  n, imp = 67, 40
  env = _make_env('point', 'go_to_goal', n_envs=n, seed=43, rgb_observation=True, device_buffers=True)
  env.reset()
  good = env._descs[0]
  bad = dict(good, extents=[-0.5, -0.5, 0.5, 0.5])   # robot within +-0.1, every hazard within +-0.3: never 0.6 apart
  doe = np.zeros(n, np.int32); doe[imp] = 1
  env._ctx[0].set_tasks([good, bad], doe, None, env_id0=0)
  rng = np.random.RandomState(4)
  for _ in range(3):
    out = env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32))
  before, pre = _np(out[0]).copy(), env.get_state()
  m = rng.rand(n) < 0.4
  m[imp] = True
  feasible = m.copy(); feasible[imp] = False
  img = env.reset(mask=m, sync=False)
  assert env.reset_counts() == (int(feasible.sum()), 1)   # (joins the stream)
  got, post = _np(img), env.get_state()
  np.testing.assert_array_equal(post[0][~feasible], pre[0][~feasible])
  assert post[1][imp, R.I_FLAGS] & 1 and not pre[1][imp, R.I_FLAGS] & 1
  np.testing.assert_array_equal(got[~feasible], before[~feasible], err_msg='rows of the kept envs and of the impossible one')
  np.testing.assert_array_equal(got, env._ctx[0].render_rgb())
  assert (got[feasible] != before[feasible]).any(axis=(1, 2, 3)).all()
  env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
class _NoDevice:
  """Stands in for _native.Context where only the constructor's and render()'s argument checks run: any other use fails."""
  CAMERAS = {'vision': 0, 'fixednear': 1, 'fixedfar': 2, 'track': 3}

  def __init__(self, robot, n_envs, device=0, seed=0):
    self.robot, self.n_envs, self.device = robot, n_envs, device

  def set_seed(self, seed):
    pass

  def close(self):
    pass


@pytest.fixture
def sag_no_device(monkeypatch):
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import envs
  monkeypatch.setattr(envs.nat, 'Context', _NoDevice)
  return sag


def test_episode_loop_accepts_images(sag_no_device):
  """An rgb_observation env with device_buffers and device_reset takes time_limit / auto_reset through episode_loop(); the
  loop still refuses parity_rng and missing device_buffers / device_reset, from make() and from episode_loop() alike, and a
  refused call leaves the env as it was."""
  sag = sag_no_device
  dev = {'device_buffers': True, 'device_reset': True}
  for kw in ({'time_limit': 5}, {'auto_reset': True}, {'time_limit': 5, 'auto_reset': True}):
    env = sag.make('point', None, n_envs=8, rgb_observation=True, **dev)
    assert env.observation_space.shape == (64, 64, 3) and not env._track
    env.episode_loop(**kw)
    assert env._track and env.time_limit == kw.get('time_limit') and env.auto_reset == bool(kw.get('auto_reset'))
    env.episode_loop()
    assert not env._track
    env.close()
    for rgb in (False, True):
      for base in ({}, {'device_buffers': True}, {'device_reset': True}):
        env = sag.make('point', None, n_envs=8, rgb_observation=rgb, **base)
        with pytest.raises(ValueError):
          env.episode_loop(**kw)
        assert not env._track and env.time_limit is None and not env.auto_reset
        if not rgb:
          with pytest.raises(ValueError):
            sag.make('point', None, n_envs=8, **base, **kw)
    for base in (dict(dev, parity_rng=True), {'parity_rng': True}):
      with pytest.raises(ValueError):
        sag.make('point', None, n_envs=8, **base, **kw)
  env = sag.make('point', None, n_envs=8, rgb_observation=True, **dev)
  with pytest.raises(ValueError):
    env.episode_loop(time_limit=0)
  assert not env._track


def test_reset_async_with_images_still_needs_device_buffers_and_device_reset(sag_no_device):
  from safe_adaptation_gym_amd import benchmark
  sag = sag_no_device
  for base in ({}, {'device_buffers': True}, {'device_reset': True}):
    env = sag.make('point', None, n_envs=8, rgb_observation=True, **base)
    env._tasks = [benchmark.TASKS['go_to_goal']() for _ in range(8)]   # (set_task would sample on the device)
    with pytest.raises(ValueError, match='needs device_buffers=True and device_reset=True'):
      env.reset(sync=False)
  env = sag.make('point', None, n_envs=8, rgb_observation=True, device_buffers=True, device_reset=True)
  env._tasks = [benchmark.TASKS['go_to_goal']() for _ in range(8)]
  with pytest.raises(ValueError, match='new task'):
    env.reset(sync=False, options={'task': benchmark.TASKS['go_to_goal']})


def test_render_envs_argument_checks_without_a_device(sag_no_device):
  """render(envs=...) refuses what is not a 1-D integer list of indices in [0, n_envs) before it touches a context (the
  stand-in context has no render at all); an empty list needs no context either."""
  env = sag_no_device.make('point', None, n_envs=8, devices=[0, 0])
  for bad in (np.zeros(8, bool), [True, False], np.array([0.0, 1.0]), [[0, 1]], np.zeros((2, 2), np.int32), [-1], [8], [0, 3, 8], 3):
    with pytest.raises(ValueError):
      env.render(envs=bad)
  with pytest.raises(KeyError):
    env.render(envs=[0], camera_id='nowhere')
  assert env.render(envs=[], width=5, height=4).shape == (0, 4, 5, 3)
  with pytest.raises(AttributeError):
    env.render(envs=[0])   # a valid list goes on to the context

"""final_observation=True: the observation rows of the envs that end an episode under auto_reset, kept before the stream-ordered
reset overwrites them.  The masked row copy itself (k_save_rows of csrc/sag_rollout.hpp through sag_copy_rows_device) against
np.where, byte for byte; then the env switch against the loop written by hand the way step()'s docstring described it
before the switch existed - step with time_limit alone, read the observation, reset(mask=done, sync=False): two paths through
the same kernels on the same device, so every comparison is exact."""
import numpy as np
import pytest

from test_device_reset import KEY
from test_reset_loop import _m_bytes, _m_first, _m_last, _m_ones, _m_random, _m_zeros, _make_env, _np
from test_rgb_rollout import _NoDevice

ERR_ARG = -1   # SAG_ERR_ARG
N_ROWS = 130   # two full wavefronts and a partial one of two lanes


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(nat):
  c = nat.Context('point', N_ROWS, seed=KEY)
  yield c
  c.close()


def _m_wave(n, rng, out): return ((np.arange(n) >= 64) & (np.arange(n) < 128)).astype(np.uint8)


MASKS = {'zeros': _m_zeros, 'ones': _m_ones, 'first': _m_first, 'last': _m_last, 'one whole wavefront': _m_wave, 'random 30 %': _m_random,
         'bytes 2 and 255': _m_bytes, 'null': None}


def _sentinel(shape):
  """A byte pattern of period 251: it repeats with no row size used here."""
  return (np.arange(int(np.prod(shape)), dtype=np.int64) % 251 + 3).astype(np.uint8).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# 1. sag_copy_rows_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('row_bytes', [16, 240, 12288], ids=['1 piece', '15 pieces', '768 pieces'])
def test_copy_rows_equals_numpy_where(ctx, row_bytes):
  """Rows of 16 B (one piece per row), 240 B (15 pieces: does not divide the 64 lanes) and 12 288 B (768: several passes per
  lane) of random bytes into a buffer of sentinel bytes, under every mask of MASKS: the result is
  np.where(mask[:, None] != 0, src, sentinel), NULL meaning every row."""
  n = N_ROWS
  rng = np.random.RandomState(row_bytes)
  src = rng.randint(0, 256, (n, row_bytes)).astype(np.uint8)
  fill = _sentinel(src.shape)
  d_src, d_dst, d_mask = ctx.dev_alloc(src.nbytes), ctx.dev_alloc(src.nbytes), ctx.dev_alloc(n)
  ctx.dev_upload(d_src, src)
  for name, kind in MASKS.items():
    m8 = np.ones(n, np.uint8) if kind is None else kind(n, rng, None)
    if name.startswith(('random', 'bytes')):
      assert 0 < (m8 != 0).sum() < n, name
    ctx.dev_upload(d_mask, m8)
    ctx.dev_upload(d_dst, fill)
    ctx.copy_rows(None if kind is None else d_mask, row_bytes, d_src, d_dst)
    ctx.wait()
    np.testing.assert_array_equal(ctx.dev_download(d_dst, src.shape, np.uint8), np.where(m8[:, None] != 0, src, fill),
                                  err_msg=f'{row_bytes} B rows, mask {name}')
    np.testing.assert_array_equal(ctx.dev_download(d_src, src.shape, np.uint8), src, err_msg=f'{row_bytes} B rows, mask {name}: the source')
  for p in (d_src, d_dst, d_mask):
    ctx.dev_free(p)


@pytest.mark.gpu
def test_copy_rows_refuses_bad_arguments(nat, ctx):
  """Every refusal of the header comment returns SAG_ERR_ARG and leaves the destination as it was: NULL d_src / d_dst,
  row_bytes <= 0 or no multiple of 16, a pointer that is not 16-byte aligned, d_src == d_dst."""
  n, rb = N_ROWS, 48
  src = np.random.RandomState(1).randint(0, 256, (n, rb)).astype(np.uint8)
  fill = _sentinel(src.shape)
  size = src.nbytes + 16   # (room for the misaligned pointers)
  d_src, d_dst, d_mask = ctx.dev_alloc(size), ctx.dev_alloc(size), ctx.dev_alloc(n)
  ctx.dev_upload(d_src, src)
  ctx.dev_upload(d_mask, np.ones(n, np.uint8))
  s, d = d_src.value, d_dst.value
  assert s % 16 == 0 and d % 16 == 0
  bad = {'NULL d_src': (rb, None, d), 'NULL d_dst': (rb, s, None), 'row_bytes 0': (0, s, d), 'row_bytes -16': (-16, s, d),
         'row_bytes 40': (40, s, d), 'row_bytes 8': (8, s, d), 'd_src + 4': (rb, s + 4, d), 'd_dst + 8': (rb, s, d + 8),
         'd_src == d_dst': (rb, d, d)}
  for what, (row_bytes, a, b) in bad.items():
    for mask in (d_mask, None):
      ctx.dev_upload(d_dst, fill)
      rc = ctx.lib.sag_copy_rows_device(ctx.h, mask, row_bytes, a, b)
      ctx.wait()
      assert rc == ERR_ARG, f'{what}: {rc}'
      np.testing.assert_array_equal(ctx.dev_download(d_dst, src.shape, np.uint8), fill, err_msg=f'{what}: the destination was written')
  with pytest.raises(nat.SagError):
    ctx.copy_rows(d_mask, 40, d_src, d_dst)
  ctx.copy_rows(d_mask, rb, d_src, d_dst)   # the context is usable after the refusals
  ctx.wait()
  np.testing.assert_array_equal(ctx.dev_download(d_dst, src.shape, np.uint8), src)
  for p in (d_src, d_dst, d_mask):
    ctx.dev_free(p)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the env switch, vector observations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('stagger', [True, False], ids=['staggered', 'in step'])
@pytest.mark.parametrize('robot,task', [('point', 'go_to_goal'), ('car', 'push_box'), ('doggo', 'go_to_goal')])
def test_final_observation_equals_the_manual_loop(nat, robot, task, stagger):
  """A = make(time_limit=3, auto_reset=True, final_observation=True).  B = make(time_limit=3), driven by hand: step, copy the
  observation, reset(mask=done, sync=False).  Same seed, same actions, ten steps.  Staggered: after the first step both take
  the same random reset(mask), so later steps end some envs or none; in step: every env ends together, the all-ones mask.
  At every step `done` is equal, A's final rows of the ended envs are B's step observation, A's other final rows are what
  they were, and A's observation is B's after its reset."""
  n, limit = 96, 3   # one full wavefront and a partial one
  kw = dict(n_envs=n, seed=53, device_buffers=True, time_limit=limit)
  A, B = _make_env(robot, task, auto_reset=True, final_observation=True, **kw), _make_env(robot, task, **kw)
  np.testing.assert_array_equal(_np(A.reset()), _np(B.reset()))
  rng = np.random.RandomState(8)
  nu, od = A.robot.nu, A.robot.obs_dim
  held = np.zeros((n, od), np.float32)
  seen = set()
  for t in range(10):
    act = rng.uniform(-1, 1, (n, nu)).astype(np.float32)
    a_obs, _, a_done, a_info = A.step(act)
    b_obs, _, b_done, _ = B.step(act)
    b_step = _np(b_obs).copy()
    done = _np(a_done)
    np.testing.assert_array_equal(done, _np(b_done), err_msg=f'step {t}: done')
    b_after = B.reset(mask=b_done, sync=False)
    B.wait()
    e = done != 0
    seen.add('none' if not e.any() else ('all' if e.all() else 'some'))
    final = _np(a_info['final_observation'])
    assert final.shape == (n, od) and final.dtype == np.float32
    np.testing.assert_array_equal(final[e], b_step[e], err_msg=f'step {t}: final rows of the ended envs')
    np.testing.assert_array_equal(final[~e], held[~e], err_msg=f'step {t}: final rows of the other envs')
    np.testing.assert_array_equal(_np(a_obs), _np(b_after), err_msg=f'step {t}: observation')
    if e.any():
      assert (final[e] != _np(a_obs)[e]).any(axis=1).all(), f'step {t}: a final row equals the first row of the new episode'
    held = final
    if t == 0 and stagger:
      m = rng.rand(n) < 0.5
      assert m[:64].any() and not m[:64].all() and m[64:].any() and not m[64:].all()
      np.testing.assert_array_equal(_np(A.reset(mask=m)), _np(B.reset(mask=m)), err_msg='observation of the staggering reset')
      np.testing.assert_array_equal(_np(a_info['final_observation']), held, err_msg='reset(mask) wrote final rows')
  assert seen >= ({'none', 'some'} if stagger else {'none', 'all'}), seen
  assert held.any(axis=1).all()   # every env ended an episode
  assert A.reset_counts()[1] == 0 and B.reset_counts()[1] == 0
  A.close(); B.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the env switch, images
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_final_observation_with_images_equals_the_manual_loop(nat):
  """rgb_observation: A gets episode_loop(time_limit=2, auto_reset=True, final_observation=True), B episode_loop(time_limit=2)
  and the manual loop - its step image is the final observation.  Five steps, staggered after the first."""
  n = 8
  kw = dict(n_envs=n, seed=59, rgb_observation=True, device_buffers=True)
  A, B = _make_env('point', 'go_to_goal', **kw), _make_env('point', 'go_to_goal', **kw)
  A.episode_loop(time_limit=2, auto_reset=True, final_observation=True)
  B.episode_loop(time_limit=2)
  np.testing.assert_array_equal(_np(A.reset()), _np(B.reset()))
  rng = np.random.RandomState(9)
  held = np.zeros((n, 64, 64, 3), np.uint8)
  partial = 0
  for t in range(5):
    act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    a_img, _, a_done, a_info = A.step(act)
    b_img, _, b_done, _ = B.step(act)
    b_step = _np(b_img).copy()
    done = _np(a_done)
    np.testing.assert_array_equal(done, _np(b_done), err_msg=f'step {t}: done')
    b_after = B.reset(mask=b_done, sync=False)
    B.wait()
    e = done != 0
    partial += int(e.any() and not e.all())
    final = _np(a_info['final_observation'])
    assert final.shape == (n, 64, 64, 3) and final.dtype == np.uint8
    np.testing.assert_array_equal(final[e], b_step[e], err_msg=f'step {t}: final images of the ended envs')
    np.testing.assert_array_equal(final[~e], held[~e], err_msg=f'step {t}: final images of the other envs')
    np.testing.assert_array_equal(_np(a_img), _np(b_after), err_msg=f'step {t}: images')
    held = final
    if t == 0:
      m = np.arange(n) % 2 == 1
      np.testing.assert_array_equal(_np(A.reset(mask=m)), _np(B.reset(mask=m)), err_msg='images of the staggering reset')
  assert partial >= 2, partial
  assert held.any(axis=(1, 2, 3)).all()
  A.close(); B.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def sag_no_device(monkeypatch):
  """make() with a stand-in for _native.Context (test_rgb_rollout._NoDevice): the switches are checked before a context is used."""
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import envs
  monkeypatch.setattr(envs.nat, 'Context', _NoDevice)
  return sag


DEV = {'device_buffers': True, 'device_reset': True}


def _switches(env):
  return env.time_limit, env.auto_reset, env.final_observation, env._track


def test_final_observation_needs_auto_reset(sag_no_device):
  sag = sag_no_device
  for kw in ({}, {'time_limit': 5}, {'auto_reset': False}):
    with pytest.raises(ValueError, match='auto_reset'):
      sag.make('point', None, n_envs=8, final_observation=True, **DEV, **kw)
    env = sag.make('point', None, n_envs=8, **DEV)
    with pytest.raises(ValueError, match='auto_reset'):
      env.episode_loop(final_observation=True, **kw)
    assert _switches(env) == (None, False, False, False)
  for kw in ({'auto_reset': True}, {'time_limit': 5, 'auto_reset': True}):
    env = sag.make('point', None, n_envs=8, final_observation=True, **DEV, **kw)
    assert _switches(env) == (kw.get('time_limit'), True, True, True)
    env = sag.make('point', None, n_envs=8, **DEV, **kw)
    assert not env.final_observation   # the default is off
    env.episode_loop(final_observation=True, **kw)
    assert _switches(env) == (kw.get('time_limit'), True, True, True)
    env.episode_loop(**kw)
    assert _switches(env) == (kw.get('time_limit'), True, False, True)
  # the loop's own requirements hold with the switch on
  for base in ({}, {'device_buffers': True}, {'device_reset': True}, dict(DEV, parity_rng=True)):
    with pytest.raises(ValueError):
      sag.make('point', None, n_envs=8, auto_reset=True, final_observation=True, **base)


def test_refused_episode_loop_keeps_the_switches(sag_no_device):
  sag = sag_no_device
  env = sag.make('point', None, n_envs=8, time_limit=5, auto_reset=True, final_observation=True, **DEV)
  before = _switches(env)
  assert before == (5, True, True, True)
  for kw in ({'final_observation': True}, {'time_limit': 7, 'final_observation': True}, {'time_limit': 0, 'auto_reset': True, 'final_observation': True}):
    with pytest.raises(ValueError):
      env.episode_loop(**kw)
    assert _switches(env) == before, kw
  env = sag.make('point', None, n_envs=8, time_limit=5, auto_reset=True, **DEV)
  with pytest.raises(ValueError):
    env.episode_loop(time_limit=7, final_observation=True)
  assert _switches(env) == (5, True, False, True)


def test_image_envs_take_the_switch_through_episode_loop(sag_no_device):
  sag = sag_no_device
  with pytest.raises(ValueError, match='episode_loop'):
    sag.make('point', None, n_envs=8, rgb_observation=True, auto_reset=True, final_observation=True, **DEV)
  with pytest.raises(ValueError):
    sag.make('point', None, n_envs=8, rgb_observation=True, final_observation=True, **DEV)
  env = sag.make('point', None, n_envs=8, rgb_observation=True, **DEV)
  with pytest.raises(ValueError, match='auto_reset'):
    env.episode_loop(time_limit=2, final_observation=True)
  assert _switches(env) == (None, False, False, False)
  env.episode_loop(time_limit=2, auto_reset=True, final_observation=True)
  assert _switches(env) == (2, True, True, True)

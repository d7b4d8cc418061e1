"""The observation rows sag_step_device writes (step_body's epilogue, csrc/sag_device.hpp), checked against things that
do not share its code: a buffer pre-filled with a bit pattern no step produces and guarded by rows the step must leave
alone, the columns whose values are known constants, and the oracle.  The equality tests of test_gpu_parity.py compare the
single-launch form with the split form, which stage and store their rows with the same code; these do not.

Point / go_to_goal has neither buttons nor a task object: its kernels stage the whole 60-column row in LDS and write it
in one store phase (obs_whole_rows).  Car / push_box keeps the chunk-by-chunk path.  The batches are far below the
threshold of four wavefronts per CU, so the single-launch form runs with 16 envs per wavefront; 193 envs leave a partial
last wavefront, and in the split form holes in the quiet launch and scattered rows in the busy one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import _flags_agree, _lidar_e2e_bound, _rows_off, _state_tol, nat, oracle  # noqa: F401 (fixtures)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7fa5c3e1)   # a NaN with a payload: no arithmetic of the step yields these bits
GUARD_ROWS = 2                     # rows of the buffer before and after the live rows


class _GuardedRun:
  """bench.DeviceRun whose observation pointer sits GUARD_ROWS rows (+ byte_off bytes) inside a larger device buffer."""

  def __init__(self, monkeypatch, n, split, byte_off=0, robot='point', task='go_to_goal', crowd=False):
    monkeypatch.setenv('SAG_SPLIT', split)
    self.run = bench.DeviceRun(task, n, 0, 0, robot=robot)
    if crowd:
      # Fresh layouts keep every robot clear of the objects, so a batch this small is all quiet from its second step on:
      # the robot of every third env goes right next to its first vase, which keeps that env busy.
      from safe_adaptation_gym_amd import _native as nat
      rf, ri = self.run.ctx.get_state()
      ids = np.arange(0, n, 3, dtype=np.int32)
      ids = ids[ri[ids, nat.I_NV] > 0]
      rf[ids, nat.F_ROBOT] = rf[ids, nat.F_VASES] + rf[ids, nat.F_VASE_SIZE] + np.float32(0.1)
      rf[ids, nat.F_ROBOT + 1] = rf[ids, nat.F_VASES + 1]
      self.run.ctx.set_state(rf[ids], ri[ids], ids)
    self.n, self.od = n, self.run.ctx.info['obs_dim']
    self.words = (n + 2 * GUARD_ROWS) * self.od + 4
    self.first = GUARD_ROWS * self.od + byte_off // 4
    self.buf = self.run.ctx.dev_alloc(self.words * 4)
    assert byte_off % 4 == 0 and byte_off < 16
    self.run.d_obs = C.c_void_p(self.buf.value + GUARD_ROWS * self.od * 4 + byte_off)

  def step(self):
    """One step into the sentinel-filled buffer -> the live rows as uint32 [n, obs_dim], guards checked."""
    c = self.run.ctx
    c.dev_upload(self.buf, np.full(self.words, SENTINEL, np.uint32))
    self.run.step()
    c.wait()
    w = c.dev_download(self.buf, (self.words,), np.uint32)
    live = w[self.first:self.first + self.n * self.od].reshape(self.n, self.od)
    assert (w[:self.first] == SENTINEL).all(), 'the rows in front of the batch were written'
    assert (w[self.first + self.n * self.od:] == SENTINEL).all(), 'the rows behind the batch were written'
    bad = np.argwhere(live == SENTINEL)
    assert len(bad) == 0, f'{len(bad)} elements never written, first (env, column) {bad[0].tolist()}'
    return live

  def close(self):
    self.run.ctx.dev_free(self.buf)
    self.run.close()


def _check_constants(bits, objects_empty):
  obs = bits.view(np.float32)
  if objects_empty:
    assert (bits[:, 16:32] == 0).all(), 'the objects chunk of an instance without objects is +0.0'
  assert (obs[:, 50] == np.float32(9.81)).all(), 'accelerometer z'
  assert (obs[:, [53, 54, 55, 59]] == 0).all(), 'velocimeter z, gyro x / y, magnetometer z'


@pytest.mark.parametrize('split', ['0', '1'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 193])
def test_sentinel_and_guard_rows(nat, monkeypatch, n, split):
  """Three steps into a NaN-filled buffer with guard rows: every element of every live row is written, nothing else is,
  the empty objects chunk is +0.0 and the constant sensor columns hold their constants.  193 envs in the split form: both
  launches take part (0 < busy envs < N) by the third step, or as soon after as the seeded layout gives it."""
  g = _GuardedRun(monkeypatch, n, split, crowd=n == 193)
  for _ in range(3):
    _check_constants(g.step(), True)
  if n == 193 and split == '1':
    steps = 3
    while not 0 < g.run.ctx.busy_count() < n:
      assert steps < 40, f'after {steps} steps the batch is still all busy or all quiet ({g.run.ctx.busy_count()} busy)'
      _check_constants(g.step(), True)
      steps += 1
    print(f'193 envs: step {steps} ran {g.run.ctx.busy_count()} envs in the busy launch, the rest in the quiet one')
  g.close()


@pytest.mark.parametrize('n', [65, 193])
def test_rows_against_the_oracle(nat, oracle, monkeypatch, n):
  """20 steps of the split form against the oracle's step from the device's pre-step state, with the tolerances and
  helpers of test_bench_device_run_vs_oracle: a row or a column stored in the wrong place fails them grossly."""
  g = _GuardedRun(monkeypatch, n, '1')
  ctx, tol = g.run.ctx, _state_tol(nat, 'point')
  for t in range(20):
    rf, ri = ctx.get_state()
    arr = oracle.make_batch(rf, ri)
    acts = np.array([oracle.actions((666, 0), int(e), t % bench.N_ACTION_BUFS, 2) for e in ri[:, nat.I_ENV_ID]], np.float32)
    d_obs = g.step().view(np.float32)
    o_obs = oracle.step_batch_full(arr, 0, acts, key=(666, 0))[0]
    d_rf, _ = ctx.get_state()
    o_rf, _ = oracle.batch_records(arr)
    ok = ~_rows_off(d_rf, o_rf, tol)
    assert ok.mean() > 0.99, f'step {t}: {int((~ok).sum())} envs outside the state tolerance'
    e2e = _lidar_e2e_bound(nat, d_rf, o_rf)
    worst = np.abs(d_obs[ok, :48] - o_obs[ok, :48]).max(1) - e2e[ok]
    assert (worst <= 0).all(), f'lidar e2e step {t}'
    np.testing.assert_allclose(d_obs[ok, 50:], o_obs[ok, 50:], rtol=2e-4, atol=2e-4, err_msg=f'sensors step {t}')
  g.close()


@pytest.mark.parametrize('split', ['0', '1'])
def test_misaligned_pointer_equals_aligned(nat, monkeypatch, split):
  """An observation pointer 4 bytes off a 16-byte boundary takes the dword path: same guards, and the values of the
  aligned run bit for bit."""
  a, b = _GuardedRun(monkeypatch, 65, split), _GuardedRun(monkeypatch, 65, split, byte_off=4)
  for t in range(3):
    ra, rb = a.step(), b.step()
    _check_constants(rb, True)
    np.testing.assert_array_equal(ra, rb, err_msg=f'step {t}')
  a.close()
  b.close()


@pytest.mark.parametrize('split', ['0', '1'])
def test_sentinel_and_guard_rows_car_push_box(nat, monkeypatch, split):
  """Car / push_box, 65 envs: 72 columns and a task object, so the objects chunk is not empty."""
  g = _GuardedRun(monkeypatch, 65, split, robot='car', task='push_box')
  assert g.od == 72
  for _ in range(3):
    _check_constants(g.step(), False)
  g.close()

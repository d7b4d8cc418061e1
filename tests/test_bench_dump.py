"""bench.py --dump-outputs on a CPU stand-in for DeviceRun: what is written is the last timed step's output, --steps sets
the number of timed steps, the env sample is fixed and within the byte budget; a plain run makes the headline's run only and
--full adds the others.  The harness is tested, not the kernel."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class CountingRun:
  """DeviceRun's interface; the outputs of a step are a function of (env, steps taken so far)."""

  made = []   # (robot, task, envs) of every run created

  def __init__(self, task, envs, device, rank, robot='point'):
    self.envs, self.t = envs, 0
    CountingRun.made.append((robot, task, envs))

  def burn_in(self, steps):
    self.run(steps)

  def run(self, steps):
    self.t += steps

  def wait(self):
    pass

  def timing(self, on):
    pass

  def kernel_time_ms(self):
    return 1.0, self.t

  def stats(self):
    return 0.0, 0, True

  def outputs(self):
    e = np.arange(self.envs, dtype=np.float32)
    return {'obs': e[:, None] * 100 + np.arange(60, dtype=np.float32) + self.t * 1e-2,
            'reward': np.stack([e, -e], 1) + self.t, 'cost': (np.arange(self.envs) % 2).astype(np.uint8),
            'done': np.zeros(self.envs, np.uint8), 'goal_met': np.full(self.envs, self.t % 256, np.uint8)}

  def close(self):
    pass


def _bench(out_dir, envs, steps):
  lines = []
  bench.main(['--steps', str(steps), '--warmup', '3', '--burn-in', '2', '--envs', str(envs), '--no-c2', '--no-c4',
              '--no-cpu-baseline', '--dump-outputs', str(out_dir)], run_factory=CountingRun, emit=lines.append)
  assert len(lines) == 1
  return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def _last_step(envs, steps):
  ref = CountingRun('go_to_goal', envs, 0, 0)
  ref.run(2 + 3 + steps)   # burn-in + warmup + --steps
  return ref.outputs()


def test_dump_is_the_last_timed_step(tmp_path):
  res, d = _bench(tmp_path, 500, 7)
  assert res['steps'] == 7
  assert set(d) == {'env_id', 'obs', 'reward', 'cost', 'done', 'goal_met'}
  assert d['env_id'].dtype == np.float64 and all(d[k].dtype == np.float32 for k in d if k != 'env_id')
  np.testing.assert_array_equal(d['env_id'], np.arange(500))   # 500 envs fit the budget: no sampling
  for k, a in _last_step(500, 7).items():
    np.testing.assert_array_equal(d[k], a.astype(np.float32))


def test_dump_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, 'DUMP_BYTES', 64 << 10)
  _, a = _bench(tmp_path / 'a', 5000, 4)
  _, b = _bench(tmp_path / 'b', 5000, 4)
  ids = a['env_id']
  assert 0 < len(ids) < 5000 and np.all(np.diff(ids) > 0) and ids[-1] < 5000
  assert sum(x.nbytes for x in a.values()) <= 64 << 10
  for k in a:
    np.testing.assert_array_equal(a[k], b[k])
  for k, x in _last_step(5000, 4).items():
    np.testing.assert_array_equal(a[k], x[ids.astype(np.int64)].astype(np.float32))


HEADLINE_KEYS = {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'}
EXTRA_KEYS = {'c2_4096_envs', 'c2_lidar_cost_only', 'c3_car_push_box', 'c4_doggo_multitask', 'c5_doggo_haul_box_rgb_4096', 'cpu_baseline'}


def _plain(argv, monkeypatch):
  """bench.main(argv) on the stand-in; the CPU baseline is not a run object, so it is caught where it would start."""
  baselines = []
  monkeypatch.setattr(bench, 'cpu_baseline', lambda *a, **k: baselines.append(a) or {'value': 0.0})
  CountingRun.made, lines = [], []
  bench.main(argv, run_factory=CountingRun, emit=lines.append)
  assert len(lines) == 1
  return json.loads(lines[0]), list(CountingRun.made), baselines


def test_plain_run_measures_the_headline_only(monkeypatch):
  res, made, baselines = _plain(['--gpus', '1', '--steps', '5', '--warmup', '3', '--burn-in', '2', '--envs', '64'], monkeypatch)
  assert made == [('point', 'go_to_goal', 64)] and baselines == []
  assert HEADLINE_KEYS <= set(res) and not EXTRA_KEYS & set(res)
  assert res['metric'] == 'env-steps/sec (batched) Point/GoToGoal' and res['unit'] == 'env-steps/s' and res['dtype'] == 'f32'
  assert res['higher_is_better'] is True and res['steps'] == 5 and res['warmup'] == 3
  assert abs(res['value'] - 64 * 5 / (res['ms_per_step'] * 5e-3)) < 1e-6 * res['value']
  # the switches that trim a --full run change nothing without it
  res2, made2, baselines2 = _plain(['--steps', '5', '--warmup', '3', '--burn-in', '2', '--envs', '64', '--no-c2', '--no-c4', '--no-cpu-baseline'], monkeypatch)
  assert made2 == made and baselines2 == [] and set(res2) == set(res)


def test_full_adds_the_other_lines(monkeypatch):
  plain, _, _ = _plain(['--steps', '5', '--warmup', '3', '--burn-in', '2', '--envs', '64'], monkeypatch)
  res, made, _ = _plain(['--full', '--steps', '5', '--warmup', '3', '--burn-in', '2', '--envs', '64', '--c4-envs', '12', '--c4-steps', '2'], monkeypatch)
  # on a stand-in only the sharded Doggo / multitask line follows (the single-GPU lines and the CPU baselines need DeviceRun)
  assert made == [('point', 'go_to_goal', 64), ('doggo', 'multitask', 12)]
  assert set(res) == set(plain) | {'c4_doggo_multitask'} and res['c4_doggo_multitask']['steps'] == 2
  _, made, _ = _plain(['--full', '--no-c4', '--steps', '5', '--warmup', '3', '--burn-in', '2', '--envs', '64'], monkeypatch)
  assert made == [('point', 'go_to_goal', 64)]

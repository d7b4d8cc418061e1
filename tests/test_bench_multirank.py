"""The N>1 path of bench.py (sharding by env index, barrier, max over ranks, one JSON line
from rank 0) under torch.distributed/gloo with world_size 2 on CPU.  The GPU stepper is
replaced by the CPU oracle here - the only place outside bench's cpu_baseline leg where that
is allowed - so what is tested is the harness, not the kernel."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, os, sys, time
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np
import bench
from oracle_lib import Oracle

class OracleRun:
  """CPU stand-in with DeviceRun's interface."""
  def __init__(self, task, envs, device, rank, robot='point'):
    self.o = Oracle()
    rf, ri = bench.build_records(task, envs, rank, robot=robot)
    self.rid, self.nu, self.od = {'point': (0, 2, 60), 'car': (1, 2, 72), 'doggo': (2, 12, 104)}[robot]
    self.robot = robot
    self.ids = ri[:, 12].copy()
    self.tasks = sorted(set(int(x) for x in ri[:, 0]))
    self.arr = self.o.make_batch(rf, ri)
    self.envs, self.t, self.rank = envs, 0, rank
    self.acts = np.stack([[self.o.actions((666, 0), int(i), s, self.nu) for i in self.ids] for s in range(2)])
    self.ms, self.n = 0.0, 0
  def burn_in(self, steps): self.run(steps)
  def run(self, steps):
    for _ in range(steps):
      t0 = time.perf_counter()
      self.out = self.o.step_batch(self.arr, self.rid, self.acts[self.t %% 2], key=(666, 0), obs_dim=self.od)
      self.ms += (time.perf_counter() - t0) * 1e3; self.n += 1; self.t += 1
      if self.rank == 1: time.sleep(0.002)   # a slower rank: the max over ranks must see it
  def wait(self): pass
  def timing(self, on): self.ms, self.n = 0.0, 0
  def kernel_time_ms(self): return (self.ms / max(self.n, 1), self.n)
  def stats(self): return float(self.out[2].mean()), int(self.out[3].sum()), bool(np.isfinite(self.out[0]).all())
  def close(self):
    json.dump({'rank': self.rank, 'ids': [int(self.ids[0]), int(self.ids[-1])], 'steps': self.t, 'tasks': self.tasks},
              open(os.path.join(%(out)r, 'rank%%d_%%s.json' %% (self.rank, self.robot)), 'w'))

# a slow rendezvous: every barrier of rank 1 arrives 300 ms late.  The reported time is each rank's own K steps (clock
# stopped BEFORE the closing barrier), max-reduced - the barrier's latency must not be in it (VERDICT r3 item 9).
import torch.distributed as _dist
_barrier = _dist.barrier
def _late_barrier(*a, **k):
  if int(os.environ['RANK']) == 1: time.sleep(0.3)
  return _barrier(*a, **k)
_dist.barrier = _late_barrier

lines = []
bench.main(['--gpus', '2', '--steps', '6', '--warmup', '2', '--burn-in', '1', '--envs', '48',
            '--full', '--no-cpu-baseline', '--no-c2', '--c4-envs', '12', '--c4-steps', '2'], run_factory=OracleRun, emit=lines.append)
if int(os.environ['RANK']) == 0:
  open(os.path.join(%(out)r, 'line.json'), 'w').write('\n'.join(lines))
else:
  assert lines == []
'''


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def test_two_rank_gloo_bench(tmp_path):
  script = tmp_path / 'worker.py'
  script.write_text(WORKER % {'root': ROOT, 'out': str(tmp_path)})
  env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='1')
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
         '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), str(script)]
  r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  lines = (tmp_path / 'line.json').read_text().strip().splitlines()
  assert len(lines) == 1, 'rank 0 prints exactly one JSON line'
  res = json.loads(lines[0])
  assert res['n_gpus'] == 2 and res['steps'] == 6 and res['warmup'] == 2
  assert res['scaling'] == 'weak' and res['higher_is_better'] is True and res['vs_baseline'] is None
  assert res['config']['global_envs'] == 96 and res['config']['envs_per_gpu'] == 48
  # value = ALL ranks' env-steps / max-over-ranks time
  assert abs(res['value'] - 96 * 6 / (res['ms_per_step'] * 6e-3)) < 1e-6 * res['value']
  # the slow rank sleeps 2 ms per step: the max over ranks cannot be below that
  assert res['ms_per_step'] >= 2.0
  # ... and the 300 ms by which rank 1 is late at every barrier are NOT in the 6-step window (they would be 50 ms per step;
  # a step of the stand-in takes ~3 ms)
  assert res['ms_per_step'] < 40.0, res['ms_per_step']
  for k in ('roofline', 'config', 'metric', 'unit', 'dtype', 'data'):
    assert k in res
  assert set(res['roofline']) >= {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'}
  # shards are disjoint contiguous env-id ranges and every rank ran burn-in + warmup + K steps
  r0 = json.loads((tmp_path / 'rank0_point.json').read_text())
  r1 = json.loads((tmp_path / 'rank1_point.json').read_text())
  assert r0['ids'] == [0, 47] and r1['ids'] == [48, 95]
  assert r0['steps'] == r1['steps'] == 1 + 2 + 6
  # BASELINE config 4 is the config that names 8 GPUs: the sharded Doggo / multitask line is part of every --gpus N --full run
  c4 = res['c4_doggo_multitask']
  assert c4['n_gpus'] == 2 and c4['envs_per_gpu'] == 12 and c4['global_envs'] == 24 and c4['scaling'] == 'weak'
  assert c4['env_id_ranges_per_rank'] == [[0, 12], [12, 24]] and len(c4['kernel_ms_per_rank']) == 2
  assert abs(c4['value'] - 24 * 2 / (c4['ms_per_step'] * 2e-3)) < 1e-6 * c4['value'] and c4['ms_per_step'] >= 2.0
  assert c4['ms_per_step'] < 100.0, 'a 300-ms barrier inside the 2-step window would be 150 ms per step (the stand-in takes ~30)'
  d0 = json.loads((tmp_path / 'rank0_doggo.json').read_text())
  d1 = json.loads((tmp_path / 'rank1_doggo.json').read_text())
  assert d0['ids'] == [0, 11] and d1['ids'] == [12, 23] and d0['steps'] == d1['steps'] == 20 + 5 + 2
  assert len(set(d0['tasks']) | set(d1['tasks'])) >= 5, 'the multitask sampler mixes the tasks over the shards'


def test_shard_ranges():
  from safe_adaptation_gym_amd.envs import shard_ranges
  assert shard_ranges(10, 3) == [(0, 4), (4, 7), (7, 10)]
  assert shard_ranges(4096 * 8, 8)[-1] == (4096 * 7, 4096 * 8)
  r = shard_ranges(5, 8)
  assert r[0] == (0, 1) and r[-1] == (5, 5)


def test_roofline_blocks_are_checked_against_the_committed_profile(monkeypatch):
  """bench.checked(): a block whose kernel the profile of THESE sources lacks is refused (replaced by the reason); one it
  holds carries the profile's figures; a profile of other sources is reported as such and checks nothing."""
  sys.path.insert(0, ROOT)
  import bench
  sha = bench.source_sha16()
  prof = {'src_sha16': sha, 'summary': 'profiles/rXX_all_summary.txt',
          'kernels': {'void sag::k_step_quiet<0, false, false>(sag::StepArgs)': {'calls': 10, 'avg_us': 900.0},
                      'sag::k_compact(int const*, int, int, int*, int*, int*)': {'calls': 10, 'avg_us': 30.0}}}
  monkeypatch.setattr(bench, '_PROFILE', prof)
  ok = bench.roofline_block(892, 1 << 22, 0.95, ['k_compact', 'k_step_quiet<0'])
  assert ok['profile']['src_sha16'] == sha and set(ok['profile']['kernels']) == {'k_compact', 'k_step_quiet<0'}
  assert abs(ok['frac'] - 892 * (1 << 22) / 0.95e-3 / 8e12) < 1e-12
  bad = bench.roofline_block(376, 4096, 0.01, ['k_lidar_cost_team<16>'])
  assert 'refused' in bad and 'frac' not in bad and 'k_lidar_cost_team<16>' in bad['refused']
  monkeypatch.setattr(bench, '_PROFILE', dict(prof, src_sha16='0' * 16))
  other = bench.roofline_block(376, 4096, 0.01, ['k_lidar_cost_team<16>'])
  assert other['profile'] is None and 'frac' in other and 'other device sources' in other['profile_note']


def test_committed_profile_covers_every_kernel_bench_names():
  """If profiles/kernels.json is of the current device sources it must hold every kernel a bench block names - the same
  check bench.py makes at run time, here at commit time."""
  sys.path.insert(0, ROOT)
  import bench
  prof = json.load(open(os.path.join(ROOT, 'profiles', 'kernels.json')))
  if prof.get('src_sha16') != bench.source_sha16():
    pytest.skip('profiles/kernels.json was measured on other device sources (re-run tools/gpu_final.sh before the round ends)')
  names = list(prof['kernels'])
  want = (bench.step_kernels('point', 1 << 22) + bench.step_kernels('point', 4096) + bench.step_kernels('car', 1 << 22) +
          bench.step_kernels('car', 4096) + bench.step_kernels('doggo', 4096) + ['k_lidar_cost_team<16>', 'k_lidar_cost_team<4>', 'k_render_rgb'])
  missing = [k for k in want if not any(k in n for n in names)]
  assert not missing, missing
  assert prof.get('doggo_flops_per_env_step', {}).get('fp64', 0) > 1e6

"""Fork time: sag_fork_device against the only way to do the same without it - sag_get_state, a permutation of the rows on
the host, sag_set_state - at the same sizes, in the same script.

  python tools/fork_time.py [out.txt] [--reps 21] [--host-reps 3] [--only NAME]

Point / go_to_goal.  Cases:
  broadcast-4M   4096 leaders broadcast to 4 194 304 envs of one context (env i from env 1024 (i / 1024))
  feed-4M        a context of 4096 envs into a context of 4 194 304 (env i from env i / 1024)
  broadcast-64   4096 leaders x 64 in one context of 262 144 envs
Per case, after a warm-up of 3 calls: the median over --reps calls of the wall time from the call to the return of sag_wait
(the stream is idle before each call), and the median over --host-reps rounds of the host path (wall time of get_state +
NumPy row gather + set_state, each of which synchronises).  Every case is a process of its own, one at a time; the first
that fails ends the run.  profiles/fork_on_device.txt is such a table.

Bytes per committed env, counted from csrc/sag_fork.hpp: written 768 (the 48 float4 groups of S) + 800 (the row of the
layout store) + 16 + 4 (the int4 word and tstate) + 1 (cost byte) + 4 (decision) = 1593, + 384 of hot record in the split
form (every context from 262 144 envs on); read the same from the source (a broadcast reads each source line once from HBM
and K - 1 times from cache) + 4 (src) and, for the hot record, 304 of the state just written.  The roofline column takes
the bytes WRITTEN plus the source bytes read once per distinct source over the time, against 8 TB/s."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {'broadcast-4M': (4194304, None, 1024), 'feed-4M': (4194304, 4096, 1024), 'broadcast-64': (262144, None, 64)}
WRITTEN, HOT, READ_PER_SOURCE = 768 + 800 + 16 + 4 + 1 + 4, 384, 768 + 800 + 16 + 4 + 1
PEAK = 8e12


def child(name, reps, host_reps):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  n, n_src, k = CASES[name]

  def make(m):
    c = nat.Context('point', m, seed=12345)
    c.set_tasks([nat.task_desc_default(3)], np.zeros(m, np.int32))
    assert c.reset_device(True, 1, want_status=False, want_bound=False)[0] == 0
    return c

  c = make(n)
  s = make(n_src) if n_src else c
  nu = c.info['nu']
  act = c.dev_alloc(n * nu * 4)
  for t in range(3):   # a state that has been stepped (and, in the split form, hot records that are valid)
    c.dev_fill_actions(act, t)
    c.step_device(act)
  c.wait()
  src = (np.arange(n) // k).astype(np.int32) * (1 if n_src else k)
  d_src = c.dev_alloc(4 * n)
  c.dev_upload(d_src, src)
  ms = []
  for r in range(3 + reps):
    c.wait(); s.wait()
    t0 = time.perf_counter()
    c.fork_device(d_src, s)
    c.wait()
    ms.append((time.perf_counter() - t0) * 1e3)
  assert c.fork_counts() == (n * (3 + reps), 0)
  host = []
  for r in range(1 + host_reps):
    t0 = time.perf_counter()
    sf, si = s.get_state()
    f, i = sf[src], si[src]
    i[:, nat.I_ENV_ID] = np.arange(n, dtype=np.int32)
    c.set_state(f, i)
    host.append((time.perf_counter() - t0) * 1e3)
    del sf, si, f, i
  split = n >= 262144
  moved = n * (WRITTEN + (HOT if split else 0)) + (n // k) * READ_PER_SOURCE
  fork_ms = float(np.median(ms[3:]))
  print(json.dumps({'fork_ms': fork_ms, 'fork_min_ms': min(ms[3:]), 'host_ms': float(np.median(host[1:])), 'bytes': moved,
                    'per_env': moved / n, 'roofline': moved / (fork_ms * 1e-3) / PEAK}), flush=True)
  c.close()
  if s is not c:
    s.close()


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  reps, host_reps, only = int(opt('--reps', 21)), int(opt('--host-reps', 3)), opt('--only', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'Point / go_to_goal; wall ms from the call to the end of sag_wait, median of {reps} calls after 3 (fork) and of {host_reps} rounds '
           f'after 1 (host path: sag_get_state, NumPy row gather, sag_set_state)',
           f'{"case":<14} {"envs":>8} {"source":>8} | {"fork ms":>9} {"min":>9} {"B / env":>8} {"GB moved":>9} {"of 8 TB/s":>9} | '
           f'{"host path ms":>12} {"host / fork":>11}']
  print('\n'.join(lines), flush=True)
  for name, (n, n_src, k) in CASES.items():
    if only and name != only:
      continue
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name, str(reps), str(host_reps)], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
      sys.exit(f'{name} ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
    m = json.loads(r.stdout.strip().splitlines()[-1])
    line = (f'{name:<14} {n:>8} {n_src or "itself":>8} | {m["fork_ms"]:9.3f} {m["fork_min_ms"]:9.3f} {m["per_env"]:8.0f} {m["bytes"] / 1e9:9.2f} '
            f'{m["roofline"]:9.1%} | {m["host_ms"]:12.1f} {m["host_ms"] / m["fork_ms"]:11.0f}')
    lines.append(line)
    print(line, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, ROOT)
    child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
  else:
    main()

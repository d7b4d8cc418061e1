"""What the fused actor-critic forward costs: sag_policy_forward_device (k_policy_forward of csrc/sag_policy.hpp) on the Point,
sampling, every output written.

  python tools/policy_time.py [out.txt] [--rounds 9] [--calls 20] [--rows N]   (--rows: that size alone)

hidden 64 and 256 at 4096 and at 4 194 304 rows; every size is a process of its own, one at a time, and all figures of a size
come from ONE context.
  forward   --calls calls enqueued back to back and one sag_wait, wall time per call, the median (and the minimum) over --rounds
            rounds after 2 of warm-up.  flop = rows * 2 * (obs_dim * H + H * H + H * (nu + 2)), the network's own products (the
            head's tile carries 32 unit rows of which nu + 2 are the network's: not counted); % peak = flop / time over the 157
            TFLOP/s of the fp32-input matrix instruction.  bytes = rows * 4 * (obs_dim + nu + 3) + the parameters once: what has
            to cross HBM.
  copy      the yardstick, same process: sag_copy_rows_device under a full mask on the same 240 B rows, 2 * rows * 240 bytes.
profiles/policy_time.txt is such a table."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4096, 4194304]
HIDDEN = [64, 256]
PEAK = 157e12   # fp32-input MFMA, FLOP/s


def _timed(c, calls, rounds, fn):
  import numpy as np
  ms = []
  for r in range(2 + rounds):
    c.wait()
    t0 = time.perf_counter()
    for _ in range(calls):
      fn()
    c.wait()
    ms.append((time.perf_counter() - t0) * 1e3 / calls)
  return float(np.median(ms[2:])), min(ms[2:])


def child(n, rounds, calls):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  c = nat.Context('point', n, seed=12345)
  od, nu = c.info['obs_dim'], c.info['nu']
  gen = np.random.default_rng(1)
  b = {k: c.dev_alloc(s) for k, s in (('obs', n * od * 4), ('copy', n * od * 4), ('mask', n), ('act', n * nu * 4), ('logp', n * 4),
                                      ('value', n * 4), ('cvalue', n * 4))}
  c.dev_upload(b['obs'], gen.uniform(-1, 1, (n, od)).astype(np.float32))
  c.dev_upload(b['mask'], np.ones(n, np.uint8))
  out = {'obs_dim': od, 'nu': nu}
  for H in HIDDEN:
    count = od * H + H + H * H + H + H * (nu + 2) + (nu + 2) + nu
    prm = gen.uniform(-0.1, 0.1, count).astype(np.float32)
    prm[-nu:] = 0.5
    p = c.dev_alloc(count * 4)
    c.dev_upload(p, prm)
    draw = [0]

    def forward():
      draw[0] += 1
      c.policy_forward(n, H, p, b['obs'], 0.0, d_actions=b['act'], d_logp=b['logp'], d_value=b['value'], d_cvalue=b['cvalue'], draw=draw[0])
    out[f'h{H}'] = _timed(c, calls if n * H < 1 << 28 else max(2, calls // 4), rounds, forward)
    out[f'h{H}_flop'] = n * 2 * (od * H + H * H + H * (nu + 2))
    out[f'h{H}_bytes'] = n * 4 * (od + nu + 3) + count * 4
    v = c.dev_download(b['value'], (min(n, 4096),), np.float32)   # (the tests compare every bit: here only that the timed calls were the kernel)
    assert np.isfinite(v).all() and v.any()
    c.dev_free(p)
  out['copy'] = _timed(c, calls, rounds, lambda: c.copy_rows(b['mask'], od * 4, b['obs'], b['copy']))
  print(json.dumps(out), flush=True)
  for p in b.values():
    c.dev_free(p)
  c.close()


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  rounds, calls, rows = int(opt('--rounds', 9)), int(opt('--calls', 20)), opt('--rows', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'Point (obs_dim 60, nu 2), sampling, every output written; one context per size.  Wall ms per call, calls back to back and one '
           f'sag_wait, median (min) of {rounds} rounds after 2',
           'flop = rows * 2 * (60 H + H H + 4 H); % peak: of 157 TFLOP/s (fp32-input MFMA); bytes = rows * 260 + parameters; '
           'copy: sag_copy_rows_device, full mask, 240 B rows, bytes = 2 * rows * 240',
           f'{"rows":>8} {"hidden":>6} | {"fwd ms":>9} {"(min)":>9} {"TFLOP/s":>8} {"% peak":>7} {"MB":>9} {"TB/s":>6} | {"copy ms":>9} '
           f'{"(min)":>9} {"TB/s":>6} {"fwd/copy":>8}']
  print('\n'.join(lines), flush=True)
  for n in ([int(rows)] if rows else SIZES):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n), str(rounds), str(calls)], capture_output=True, text=True,
                       timeout=1100)
    if r.returncode != 0:
      sys.exit(f'{n} rows ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
    m = json.loads(r.stdout.strip().splitlines()[-1])
    c_ms = m['copy']
    for H in HIDDEN:
      ms, mn = m[f'h{H}']
      rate = m[f'h{H}_flop'] / (ms * 1e-3)
      line = (f'{n:>8} {H:>6} | {ms:9.4f} {mn:9.4f} {rate / 1e12:8.2f} {100 * rate / PEAK:7.2f} {m[f"h{H}_bytes"] / 1e6:9.2f} '
              f'{m[f"h{H}_bytes"] / (ms * 1e-3) / 1e12:6.2f} | {c_ms[0]:9.4f} {c_ms[1]:9.4f} {2 * n * 240 / (c_ms[0] * 1e-3) / 1e12:6.2f} {ms / c_ms[0]:8.2f}')
      lines.append(line)
      print(line, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, ROOT)
    child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
  else:
    main()

"""Throughput mode's device reset (sag_set_tasks / sag_reset_device, csrc/sag_reset.hpp) against its specification, the NumPy
restatement tests/reset_sampler_ref.py, and that restatement against the host sampler (csrc/sag_sampler.cpp).

CPU: the restatement's Philox, its layout distribution against the host sampler's, and the kernel compiled for the host
(tests/hostemu) record for record.  GPU (-m gpu): the device records, failures, masked resets, installation, determinism."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reset_sampler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hostemu'))
KEY = 0x1234567800000abc   # a key whose high word is not zero
LAST = [38, 39, 40]   # task.reset's `last` distances: computed by the install, not by the sampler
AWAKE = 15
REF_TASKS = (0, 7, 1, 10, 12, 2, 8, 3, 13)   # the nine tasks of the reference's test_layout_sampling


def _nat():
  from safe_adaptation_gym_amd import _native
  return _native


def _cfg(**kw):
  nat = _nat()
  c = nat.world_config(kw)
  return {k: getattr(c, k) for k, _ in nat.WorldConfig._fields_ if k != 'reserved'}


def _ref_batch(robot, descs, desc_of_env, cfg, gids, nonces, key, first, prev=None):
  """The restatement for a heterogeneous batch (envs grouped by descriptor)."""
  n = len(gids)
  rf, ri, st = np.zeros((n, R.REC_FLOATS), np.float32), np.zeros((n, R.REC_INTS), np.int32), np.zeros(n, np.int32)
  for d in np.unique(desc_of_env):
    m = np.flatnonzero(desc_of_env == d)
    p = None if prev is None else {k: v[m] for k, v in prev.items()}
    rf[m], ri[m], st[m] = R.sample(robot, descs[d], cfg, np.asarray(gids)[m], np.asarray(nonces)[m], key, first, p)
  return rf, ri, st


def _prev(rf, ri):
  return {'ctrl_scale': rf[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 12], 'bound': rf[:, R.F_BOUND], 'btn_state': ri[:, R.I_BTN_STATE],
          'catch_timer': ri[:, R.I_CATCH_TIMER], 'catch_cur': rf[:, R.F_CATCH + 2], 'catch_next': rf[:, R.F_CATCH + 3]}


def _assert_records(got_f, got_i, ref_f, ref_i, maxulp=0):
  keep_f = np.setdiff1d(np.arange(R.REC_FLOATS), LAST)
  keep_i = np.setdiff1d(np.arange(R.REC_INTS), [AWAKE])
  np.testing.assert_array_equal(got_i[:, keep_i], ref_i[:, keep_i])
  if maxulp:
    np.testing.assert_array_max_ulp(got_f[:, keep_f], ref_f[:, keep_f], maxulp=maxulp)
  else:
    np.testing.assert_array_equal(got_f[:, keep_f], ref_f[:, keep_f])


def _assert_installed(nat, robot, got_f, got_i):
  """What _assert_records leaves out - the `last` distances and the awake flags, computed by the install - against the
  restatement of the install (R.install_last / R.install_awake) and against a fresh context given the same records with
  sag_set_layout (the install twin): every float and int comes back identical."""
  np.testing.assert_array_max_ulp(got_f[:, LAST], R.install_last(got_f, got_i), maxulp=1)
  np.testing.assert_array_equal(got_i[:, AWAKE], R.install_awake(got_f, got_i))
  tw = nat.Context(robot, len(got_f), seed=KEY)
  tw.set_layout(got_f, got_i)
  tf, ti = tw.get_state()
  tw.close()
  np.testing.assert_array_equal(tf, got_f)
  np.testing.assert_array_equal(ti, got_i)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_philox_equals_the_oracle():
  from oracle_lib import Oracle
  o = Oracle()
  # Random123 known-answer vectors of philox4x32-10
  kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
  for ctr, key, want in kat:
    assert tuple(int(w) for w in R.philox(*ctr, *key)) == want
    assert tuple(int(w) for w in o.philox(ctr, key)) == want
  rs = np.random.RandomState(5)
  for _ in range(64):   # stream-3 counters of both kinds
    gid, nonce = int(rs.randint(2**31)), int(rs.randint(2**24))
    w1 = int(rs.randint(10000)) << 8 | int(rs.randint(30)) if rs.rand() < .5 else R.POST | int(rs.randint(0x600))
    ctr = (gid, w1, int(rs.randint(10000)), nonce << 2 | R.STREAM)
    key = (KEY & 0xffffffff, KEY >> 32)
    np.testing.assert_array_equal(np.array(R.philox(*ctr, *key), np.uint32), o.philox(ctr, key))


def _slots(rf, ri, desc):
  """x, y columns of every placement of the records (robot, hazards, vases, pillars, goal, box, buttons)."""
  cols = [(R.F_ROBOT, 'robot')]
  cols += [(R.F_HAZARDS + 2 * h, f'hazard{h}') for h in range(desc['n_hazards'])]
  cols += [(R.F_VASES + 6 * v, f'vase{v}') for v in range(desc['n_vases'])]
  cols += [(R.F_PILLARS + 2 * p, f'pillar{p}') for p in range(desc['n_pillars'])]
  if desc['has_goal']:
    cols.append((R.F_GOAL, 'goal'))
  if desc['box_kind']:
    cols.append((R.F_BOX, 'box'))
  cols += [(R.F_BUTTONS + 2 * b, f'button{b}') for b in range(desc['n_buttons'])]
  return cols


@pytest.mark.parametrize('robot', ['point', 'doggo'])
def test_restatement_follows_the_host_samplers_distribution(robot):
  nat = _nat()
  cfg = _cfg()
  n = 3000 if robot == 'point' else 1200
  it_margin = cfg['placements_margin'] + (0.165 if robot == 'doggo' else 0.0)
  for tid in range(14):
    d = nat.task_desc_default(tid)
    hf, hi, hs = nat.sample_layouts(robot, np.arange(n) + 1000 * tid, np.full(n, tid), first_episode=True)
    rf, ri, rs = R.sample(robot, d, cfg, np.arange(n) + 7 * tid, 1, KEY, True)
    if robot == 'point' and tid in REF_TASKS:
      assert (rs != 0).mean() <= 1 / 200 and (hs != 0).mean() <= 1 / 200, (tid, (rs != 0).mean(), (hs != 0).mean())
    hf, rf = hf[hs == 0].astype(np.float64), rf[rs == 0].astype(np.float64)
    for col, name in _slots(rf, ri, d):
      for off in (0, 1):
        a, b = hf[:, col + off], rf[:, col + off]
        se = np.sqrt(a.var() / len(a) + b.var() / len(b)) + 1e-12
        assert abs(a.mean() - b.mean()) < 5 * se, (tid, name, off, a.mean(), b.mean(), se)
        va = np.sqrt(((a - a.mean()) ** 4).mean() / len(a) + ((b - b.mean()) ** 4).mean() / len(b)) + 1e-12
        assert abs(a.var() - b.var()) < 5 * va, (tid, name, off, a.var(), b.var(), va)
    # every rule of the layout holds in the restatement's records (fp32 positions: 1e-5 of slack)
    it = R.Items(d, cfg, R.ROBOTS[robot])
    P = np.stack([np.stack([rf[:, c], rf[:, c + 1]], 1) for c, _ in _slots(rf, ri, d)], 1)
    for q in range(it.n):
      lo = it.rect[q, :2] + it.ko[q] - 1e-5
      hi = it.rect[q, 2:] - it.ko[q] + 1e-5
      if q not in (it.i_goal, it.i_box if d['box_at_robot'] else -1):
        assert ((P[:, q] >= np.minimum(lo, hi)) & (P[:, q] <= np.maximum(lo, hi))).all(), (tid, q)
      for p_ in range(q):
        if it.i_goal in (p_, q) or (d['box_at_robot'] and it.i_box in (p_, q)):
          continue
        dist = np.hypot(*(P[:, q] - P[:, p_]).T)
        assert (dist >= it.ko[q] + it.ko[p_] + it_margin - 1e-5).all(), (tid, q, p_)
      if it.i_goal >= 0 and q != it.i_goal:
        dist = np.hypot(*(P[:, it.i_goal] - P[:, q]).T)
        assert (dist >= it.ko[q] + d['goal_keepout'] - 1e-5).all(), (tid, q)
    if d['box_at_robot']:
      np.testing.assert_allclose(P[:, it.i_box, 0], P[:, 0, 0] + d['box_offset'], atol=1e-6)


def test_restatement_fails_every_env_of_an_impossible_config():
  cfg = _cfg(hazards_size=2.0, vases_size=2.0, pillars_size=2.0)
  d = _nat().task_desc_default(3)
  rf, ri, st = R.sample('point', d, cfg, np.arange(4), 1, KEY, True, chunk=1000)
  assert (st == -1).all() and not rf.any() and not ri.any()


HOSTEMU_RUN = r'''
import sys, numpy as np
from safe_adaptation_gym_amd import _native as nat
out, key = sys.argv[1], int(sys.argv[2])
res = {}
cases = [('point', list(range(14)), 64), ('car', [10], 64), ('doggo', [7], 64)]
if sys.argv[3:] == ['masked']:   # the masked part only (the sanitizer build)
  cases = []
for robot, tasks, per in cases:
  descs = [nat.task_desc_default(t) for t in tasks]
  doe = np.repeat(np.arange(len(tasks)), per).astype(np.int32)
  c = nat.Context(robot, len(doe), seed=key)
  c.set_tasks(descs, doe, None, env_id0=1000)
  rc0, st0, b0 = c.reset_device(True, episode0=77)
  f0, i0 = c.get_state()
  rc1, st1, b1 = c.reset_device(False)
  f1, i1 = c.get_state()
  res.update({robot + '_f0': f0, robot + '_i0': i0, robot + '_f1': f1, robot + '_i1': i1,
              robot + '_rc': np.array([rc0, rc1]), robot + '_b1': b1})
  c.close()
# a masked reset and a replay by ids on a ragged batch: the list, scatter and gather kernels (k_reset_list, k_move_rows, k_install with ids)
n = 64 * 2 + 3
descs = [nat.task_desc_default(t) for t in (3, 7, 10)]
c = nat.Context('point', n, seed=key)
c.set_tasks(descs, (np.arange(n) % 3).astype(np.int32), None, env_id0=1000)
rc0 = c.reset_device(True, episode0=77)[0]
fa, ia = c.get_state()
m = np.where(np.arange(n) * 7 % 5 < 2, 255, 0).astype(np.uint8)
m[0], m[-1] = 0, 2
p = c.dev_alloc(n)
c.dev_upload(p, m)
rc1, st1, b1 = c.reset_device(False, d_mask=p)
fb, ib = c.get_state()
c.reset(np.array([n - 1, 3, 64, 0], np.int32))
fc, ic = c.get_state()
c.dev_free(p)
c.close()
res.update(masked_m=m, masked_rc=np.array([rc0, rc1]), masked_st=st1, masked_b=b1, masked_fa=fa, masked_ia=ia, masked_fb=fb,
           masked_ib=ib, masked_fc=fc, masked_ic=ic)
np.savez(out, **res)
'''


def test_host_build_of_the_kernel_equals_the_restatement(tmp_path):
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.fail('no clang for the host build of the kernel')
  lib = hb.build('clang', False, False, [], False, False, 'var_base')   # (the build test_hostemu_variants uses)
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
  out = str(tmp_path / 'rec.npz')
  r = subprocess.run([sys.executable, '-c', HOSTEMU_RUN, out, str(KEY)], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
  z = np.load(out)
  cfg = _cfg()
  for robot, tasks, per in (('point', list(range(14)), 64), ('car', [10], 64), ('doggo', [7], 64)):
    descs = [_nat().task_desc_default(t) for t in tasks]
    doe = np.repeat(np.arange(len(tasks)), per)
    gids = 1000 + np.arange(len(doe))
    assert list(z[robot + '_rc']) == [0, 0]
    rf, ri, st = _ref_batch(robot, descs, doe, cfg, gids, np.full(len(doe), 77), KEY, True)
    assert not st.any()
    _assert_records(z[robot + '_f0'], z[robot + '_i0'], rf, ri)
    rf1, ri1, st1 = _ref_batch(robot, descs, doe, cfg, gids, np.full(len(doe), 78), KEY, False, _prev(z[robot + '_f0'], z[robot + '_i0']))
    _assert_records(z[robot + '_f1'], z[robot + '_i1'], rf1, ri1)
    np.testing.assert_array_equal(z[robot + '_b1'], rf1[:, R.F_BOUND])
  _check_masked(z, cfg)


def _check_masked(z, cfg):
  """The masked call of HOSTEMU_RUN on 64 * 2 + 3 envs: rows outside the mask untouched, rows inside the restatement's with
  what the install adds (`last`, awake flags: R.install_last / R.install_awake); the replay by ids restores what each env
  last received."""
  n = 64 * 2 + 3
  m = z['masked_m'] != 0
  assert m[-1] and not m[0] and 0 < m.sum() < n and list(z['masked_rc']) == [0, 0] and not z['masked_st'].any()
  descs = [_nat().task_desc_default(t) for t in (3, 7, 10)]
  doe, gids = np.arange(n) % 3, 1000 + np.arange(n)
  fa, ia, fb, ib, fc, ic = (z['masked_' + k] for k in ('fa', 'ia', 'fb', 'ib', 'fc', 'ic'))
  np.testing.assert_array_equal(fb[~m], fa[~m])
  np.testing.assert_array_equal(ib[~m], ia[~m])
  rf, ri, st = _ref_batch('point', descs, doe[m], cfg, gids[m], np.full(m.sum(), 78), KEY, False, _prev(fa[m], ia[m]))
  _assert_records(fb[m], ib[m], rf, ri)
  np.testing.assert_array_equal(fb[m][:, LAST], R.install_last(fb[m], ib[m]))
  np.testing.assert_array_equal(ib[m, AWAKE], R.install_awake(fb[m], ib[m]))
  np.testing.assert_array_equal(z['masked_b'], fb[:, R.F_BOUND])
  ids = np.array([n - 1, 3, 64, 0])
  want_f, want_i = fb.copy(), ib.copy()
  want_i[ids, R.I_EPISODE] += 1
  np.testing.assert_array_equal(fc, want_f)   # (no step in between: the layout an env last received is its state)
  np.testing.assert_array_equal(ic, want_i)


def test_masked_reset_kernels_on_the_sanitizer_build(tmp_path):
  """The masked part of HOSTEMU_RUN on the ASan / UBSan host build of the library's sources (tests/hostemu/run.sh's clang
  build, here in the CPU suite): the list, scatter and gather kernels index staging rows, the layout store and the SoA state
  by env id - no sanitizer report, and the same records."""
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.fail('no clang for the host build of the kernel')
  lib = hb.build('clang', False, True, [], False, False, 'san')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'),
             ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:detect_stack_use_after_return=0:halt_on_error=1',
             UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
  # the sanitizer runtime first; whatever is preloaded already stays
  env['LD_PRELOAD'] = os.pathsep.join([hb.preload('clang')] + ([os.environ['LD_PRELOAD']] if os.environ.get('LD_PRELOAD') else []))
  out = str(tmp_path / 'rec.npz')
  r = subprocess.run([sys.executable, '-c', HOSTEMU_RUN, out, str(KEY), 'masked'], env=env, capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
  assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
  _check_masked(np.load(out), _cfg())


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nat():
  nat = _nat()
  if nat.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return nat


def _ctx(nat, robot, tasks, per, key=KEY, env_id0=0, config=None):
  descs = [nat.task_desc_default(t) for t in tasks]
  doe = np.repeat(np.arange(len(tasks)), per).astype(np.int32)
  c = nat.Context(robot, len(doe), seed=key)
  c.set_tasks(descs, doe, config, env_id0=env_id0)
  return c, descs, doe


@pytest.mark.gpu
@pytest.mark.parametrize('robot', ['point', 'car', 'doggo'])
def test_device_records_equal_the_restatement(nat, robot):
  c, descs, doe = _ctx(nat, robot, range(14), 256, env_id0=4096)
  gids = 4096 + np.arange(len(doe))
  rc, st, b = c.reset_device(True, episode0=9)
  assert rc == 0 and not st.any()
  f0, i0 = c.get_state()
  rf, ri, _ = _ref_batch(robot, descs, doe, _cfg(), gids, np.full(len(doe), 9), KEY, True)
  _assert_records(f0, i0, rf, ri, maxulp=1)
  _assert_installed(nat, robot, f0, i0)
  np.testing.assert_array_equal(b, f0[:, R.F_BOUND])
  rc, st, b = c.reset_device(False)
  f1, i1 = c.get_state()
  rf1, ri1, _ = _ref_batch(robot, descs, doe, _cfg(), gids, np.full(len(doe), 10), KEY, False, _prev(f0, i0))
  _assert_records(f1, i1, rf1, ri1, maxulp=1)
  _assert_installed(nat, robot, f1, i1)
  c.close()


@pytest.mark.gpu
def test_device_records_with_ctrl_range_scale_and_random_bound(nat):
  config = {'robot_ctrl_range_scale': 0.5, 'random_bound': 1}
  c, descs, doe = _ctx(nat, 'doggo', [3, 7], 128, config=config)
  rc, st, b = c.reset_device(True, episode0=3)
  assert rc == 0
  f0, i0 = c.get_state()
  rf, ri, _ = _ref_batch('doggo', descs, doe, _cfg(**config), np.arange(len(doe)), np.full(len(doe), 3), KEY, True)
  _assert_records(f0, i0, rf, ri, maxulp=1)
  _assert_installed(nat, 'doggo', f0, i0)
  assert len(np.unique(f0[:, R.F_BOUND])) > 200 and (f0[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 12] != 1).all()
  c.close()


@pytest.mark.gpu
def test_a_million_point_layouts_keep_every_keepout(nat):
  n = 1 << 20
  c, descs, doe = _ctx(nat, 'point', [3], n)
  rc, st, b = c.reset_device(True, episode0=1)
  assert rc == 0 and not st.any()
  rf, ri = c.get_state()
  d, cfg = descs[0], _cfg()
  it = R.Items(d, cfg, 0)
  P = np.stack([np.stack([rf[:, col], rf[:, col + 1]], 1) for col, _ in _slots(rf, ri, d)], 1).astype(np.float64)
  for q in range(it.n):
    for p_ in range(q):
      thr = it.ko[q] + it.ko[p_] + (0 if it.i_goal in (p_, q) else it.margin)
      assert (np.hypot(*(P[:, q] - P[:, p_]).T) >= thr - 1e-5).all(), (q, p_)
  c.close()


@pytest.mark.gpu
def test_impossible_config_raises_and_leaves_the_state(nat):
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd.benchmark import TASKS
  from safe_adaptation_gym_amd.utils import ResamplingError
  env = sag.make('point', 'go_to_goal', n_envs=64, device_reset=True)
  env.reset()
  before = env.get_state()
  env.close()
  c, descs, doe = _ctx(nat, 'point', [3], 64, config={'hazards_size': 2.0, 'vases_size': 2.0, 'pillars_size': 2.0})
  c.set_state(*before)
  rc, st, b = c.reset_device(False)
  assert rc == 64 and (st == -1).all()
  after = c.get_state()
  np.testing.assert_array_equal(before[0], after[0])
  np.testing.assert_array_equal(before[1], after[1])
  c.close()
  env = sag.make('point', n_envs=64, device_reset=True, config={'hazards_size': 2.0, 'vases_size': 2.0, 'pillars_size': 2.0})
  with pytest.raises(ResamplingError):
    env.set_task(TASKS['go_to_goal'])
  env.close()


@pytest.mark.gpu
def test_task_object_fields_survive_a_later_episode_and_not_a_first(nat):
  c, descs, doe = _ctx(nat, 'point', [0, 8], 64)
  c.reset_device(True, episode0=1)
  rf, ri = c.get_state()
  rf[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 12] = 0.75
  rf[:, R.F_BOUND] = 3.5
  rf[:, R.F_CATCH + 2], rf[:, R.F_CATCH + 3] = 0.6, 0.3
  ri[:, R.I_BTN_STATE], ri[:, R.I_CATCH_TIMER] = 0, 4
  c.set_state(rf, ri)
  c.reset_device(False)
  f1, i1 = c.get_state()
  assert (f1[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 12] == 0.75).all() and (f1[:, R.F_BOUND] == 3.5).all()
  assert (f1[:, R.F_CATCH + 2] == np.float32(0.6)).all() and (f1[:, R.F_CATCH + 3] == np.float32(0.3)).all()
  assert (i1[:, R.I_BTN_STATE] == 0).all() and (i1[:, R.I_CATCH_TIMER] == 4).all()
  c.reset_device(True)
  f2, i2 = c.get_state()
  assert (f2[:, R.F_CTRL_SCALE:R.F_CTRL_SCALE + 12] == 1).all() and (f2[:, R.F_BOUND] == 25).all()
  assert (f2[:, R.F_CATCH + 2] == 1).all() and (i2[:, R.I_BTN_STATE] == 1).all() and (i2[:, R.I_CATCH_TIMER] == 0).all()
  c.close()


def _masked_run(device_buffers):
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import _native as nat
  n = 4096
  env = sag.make('point', 'go_to_goal', n_envs=n, device_buffers=device_buffers, device_reset=True, seed=11)
  env.reset()
  rs = np.random.RandomState(3)
  for _ in range(30):
    out = env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32))
  last_obs = out[0].numpy() if device_buffers else out[0]
  f0, i0 = env.get_state()
  m = rs.rand(n) < 0.3
  if device_buffers:
    dm = env._ctx[0].dev_alloc(n)
    env._ctx[0].dev_upload(dm, m.astype(np.uint8))
    mask = nat.DeviceArray(env._ctx[0], dm.value, (n,), np.uint8)
  else:
    mask = m
  obs = env.reset(mask=mask)
  obs = obs.numpy() if device_buffers else obs
  f1, i1 = env.get_state()
  np.testing.assert_array_equal(f1[~m], f0[~m])
  np.testing.assert_array_equal(i1[~m], i0[~m])
  np.testing.assert_array_equal(obs[~m], last_obs[~m])
  assert (i1[m, R.I_EPISODE] == i0[m, R.I_EPISODE] + 1).all() and (i1[m, R.I_STEP] == 0).all()
  d = env._descs[0]
  rf, ri, st = R.sample('point', d, _cfg(), np.flatnonzero(m), i1[m, R.I_EPISODE], env._base_seed, False, _prev(f0[m], i0[m]))
  _assert_records(f1[m], i1[m], rf, ri, maxulp=1)
  _assert_installed(nat, 'point', f1[m], i1[m])
  env.close()


@pytest.mark.gpu
@pytest.mark.parametrize('device_buffers', [False, True])
def test_masked_reset_after_steps(nat, device_buffers):
  _masked_run(device_buffers)


@pytest.mark.gpu
def test_device_layout_installs_like_set_layout_and_replays(nat):
  c, descs, doe = _ctx(nat, 'car', [10, 3], 128)
  c.reset_device(True, episode0=5)
  rf, ri = c.get_state()
  d = nat.Context('car', len(doe), seed=KEY)
  d.set_layout(rf, ri)
  f2, i2 = d.get_state()
  np.testing.assert_array_equal(f2, rf)
  np.testing.assert_array_equal(i2, ri)
  acts = np.random.RandomState(0).uniform(-1, 1, (len(doe), 2)).astype(np.float32)
  for _ in range(10):
    oc = c.step(acts)
    od = d.step(acts)
    np.testing.assert_array_equal(oc[0], od[0])
  np.testing.assert_array_equal(c.get_state()[0], d.get_state()[0])
  c.reset()   # sag_reset replays the device-drawn layout with the next nonce
  f3, i3 = c.get_state()
  np.testing.assert_array_equal(f3, rf)   # (`last` distances included: the layout store keeps the records as installed)
  ri[:, R.I_EPISODE] += 1
  np.testing.assert_array_equal(i3, ri)   # (install-time awake flags included)
  c.close(); d.close()


@pytest.mark.gpu
def test_device_reset_is_deterministic(nat):
  import safe_adaptation_gym_amd as sag
  a = sag.make('doggo', 'haul_box', n_envs=512, device_reset=True, seed=4)
  b = sag.make('doggo', 'haul_box', n_envs=512, device_reset=True, seed=4, devices=[0, 0])
  fa, fb = a.get_state(), b.get_state()
  np.testing.assert_array_equal(fa[0], fb[0])
  np.testing.assert_array_equal(fa[1], fb[1])
  a.reset(); b.reset()
  ga, gb = a.get_state(), b.get_state()
  np.testing.assert_array_equal(ga[0], gb[0])
  assert (ga[0][:, R.F_ROBOT] != fa[0][:, R.F_ROBOT]).mean() > 0.99   # two resets in a row: new layouts
  a.close(); b.close()

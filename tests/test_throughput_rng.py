"""Throughput mode's generator, specified on the oracle (CPU): the counter-based Philox4x32-10 against the Random123
known-answer vectors, the action noise as a standard normal and the synthetic bench policy as U(-1, 1).  The GPU tests
(test_gpu_parity.py, '-k throughput') hold the device to these same functions.  Also here: the check that a foreign
device action array is float32 of the shard's shape before a step reads it."""
import math

import numpy as np
import pytest

from oracle_lib import Oracle

SEED = 0x9E3779B97F4A7C15               # a context seed whose high word (key1) is not zero
KEY = (SEED & 0xffffffff, SEED >> 32)


@pytest.fixture(scope='module')
def oracle():
  return Oracle()


# Random123 kat_vectors, philox4x32_10: counter, key, expected output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answer_vectors(oracle, ctr, key, want):
  np.testing.assert_array_equal(oracle.philox(ctr, key), np.array(want, np.uint32))


def _normal_cdf(x):
  return 0.5 * np.frompyfunc(lambda v: math.erfc(-v / math.sqrt(2)), 1, 1)(x).astype(np.float64)


def _ks(x, cdf):
  x = np.sort(np.asarray(x, np.float64))
  n = len(x)
  f = cdf(x)
  return max((np.arange(1, n + 1) / n - f).max(), (f - np.arange(n) / n).max())


KS_CRIT_1E3 = 1.949   # asymptotic Kolmogorov critical value at significance 1e-3, times 1 / sqrt(n)


def test_action_noise_is_standard_normal(oracle):
  """sago_noise_ep over 2^20 draws spread over env, step and episode nonce (the ones the GPU tests set: 0, 1, 2^23,
  0xfffffe): mean and variance within 4 standard errors of 0 and 1, the Kolmogorov-Smirnov statistic below its 1e-3
  critical value, the two values of a Box-Muller pair uncorrelated, and episode e uncorrelated with episode e + 1."""
  nu = 16
  envs = [0, 1, 63, 64, 1000, 2**20 + 7, 2**31 - 1, 2**32 - 1]
  steps = [0, 1, 2, 999, 2**31, 2**32 - 1] + list(range(10, 10 + 26))
  eps = [0, 1, 2, 2**23, 0xfffffe, 0xffffff]
  z = np.zeros((len(eps), len(envs), len(steps), nu), np.float32)
  for a, ep in enumerate(eps):
    for b, env in enumerate(envs):
      for c, st in enumerate(steps):
        z[a, b, c] = oracle.noise_ep(KEY, env, st, ep, nu)
  # the distribution tests on 2^20 more: long rows (counter word 2 = pair index) over env x step x episode
  x = np.concatenate([z.ravel()] + [oracle.noise_ep(KEY, env, st, ep, 2048) for env in range(64)
                                    for st in (3, 2**31 + 1) for ep in (0, 1, 2**23, 0xfffffe)]).astype(np.float64)
  n = len(x)
  assert n >= 1_000_000
  assert np.isfinite(x).all()
  assert abs(x.mean()) < 4 / math.sqrt(n), x.mean()
  assert abs(x.var() - 1) < 4 * math.sqrt(2 / (n - 1)), x.var()
  d = _ks(x, _normal_cdf)
  assert d < KS_CRIT_1E3 / math.sqrt(n), d
  # a pair's z0 / z1 (one Philox block, two of its words: cos and sin of one angle)
  pairs = z.reshape(-1, nu // 2, 2).reshape(-1, 2).astype(np.float64)
  r = np.corrcoef(pairs[:, 0], pairs[:, 1])[0, 1]
  assert abs(r) < 4 / math.sqrt(len(pairs)), r
  # r^2 of the pair would show a shared radius: |z0| and |z1| uncorrelated too
  r_abs = np.corrcoef(np.abs(pairs[:, 0]), np.abs(pairs[:, 1]))[0, 1]
  assert abs(r_abs) < 4 / math.sqrt(len(pairs)), r_abs
  # episode e against e + 1 (the nonce sits above the stream bits of counter word 3), incl. 0xfffffe -> 0xffffff
  e_pairs = [(0, 1), (1, 2), (4, 5)]   # 0 / 1, 1 / 2, 0xfffffe / 0xffffff
  a = np.concatenate([z[i].ravel() for i, _ in e_pairs]).astype(np.float64)
  b = np.concatenate([z[j].ravel() for _, j in e_pairs]).astype(np.float64)
  r = np.corrcoef(a, b)[0, 1]
  assert abs(r) < 4 / math.sqrt(len(a)), r
  assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[4], z[5])


def test_action_noise_episode_zero_is_sago_noise(oracle):
  for env, st in ((0, 0), (7, 2**31 + 9)):
    np.testing.assert_array_equal(oracle.noise_ep(KEY, env, st, 0, 12), oracle.noise(KEY, env, st, 12))


def test_synthetic_actions_are_uniform(oracle):
  """sago_actions (stream 2, the bench's policy) over 2^20 draws: U(-1, 1) by the Kolmogorov-Smirnov statistic, mean and
  variance; never -1, and +1 only for a word whose top 24 bits are all set: (2^24 - 1) + 0.5 rounds to 2^24 in fp32
  (found by search: env 233889 at step 2^31 + 5 under KEY, word 0).  The lower end is -1 + 2^-24."""
  nu = 256
  x = np.concatenate([oracle.actions(KEY, env, st, nu) for env in range(128) for st in (0, 1, 2**31 + 5, 2**32 - 1)]
                     + [oracle.actions((666, 0), env, st, nu) for env in range(2**20 + 5, 2**20 + 69) for st in range(64)])
  x = x.astype(np.float64)
  n = len(x)
  assert n >= 1_000_000
  assert x.min() > -1 and x.max() < 1
  assert abs(x.mean()) < 4 * math.sqrt(1 / 3 / n)
  assert abs(x.var() - 1 / 3) < 4 * math.sqrt(4 / 45 / n)   # Var(X^2) = E X^4 - (E X^2)^2 = 1/5 - 1/9 for U(-1, 1)
  assert _ks(x, lambda v: (v + 1) / 2) < KS_CRIT_1E3 / math.sqrt(n)
  edge_env, edge_step = 233889, 2**31 + 5
  w = oracle.philox((edge_env, edge_step, 0, 2), KEY)
  assert w[0] >> 8 == 0xffffff, 'the edge case is a word whose top 24 bits are set'
  assert oracle.actions(KEY, edge_env, edge_step, 2)[0] == np.float32(1), 'the one word that maps to +1'
  w = oracle.philox((5214355, edge_step, 0, 2), KEY)
  assert w[1] >> 8 == 0
  assert oracle.actions(KEY, 5214355, edge_step, 2)[1] == np.float32(-1 + 2**-24)


def test_synthetic_actions_layout(oracle):
  """Action j of an env is word j % 4 of the Philox block (env, step, j // 4, 2)."""
  for nu in (2, 3, 12):
    a = oracle.actions(KEY, 9, 2**31 + 1, nu)
    for j in range(nu):
      w = oracle.philox((9, 2**31 + 1, j // 4, 2), KEY)[j % 4]
      assert a[j] == np.float32((np.float32(w >> 8) + np.float32(0.5)) * np.float32(2.0 / 16777216.0)) - np.float32(1)


# ------------------------------------------------------------------------------------------------------------------
# foreign device actions: checked before any launch
# ------------------------------------------------------------------------------------------------------------------
class _Fake:
  """An object that exports __cuda_array_interface__ (as a torch / cupy array does), optionally with a .device."""

  def __init__(self, shape, typestr='<f4', strides=None, device=None):
    self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (0x7f0000001000, False),
                                     'version': 2, 'strides': strides}
    if device is not None:
      self.device = device


class _TorchDevice:
  def __init__(self, index):
    self.type, self.index = 'cuda', index


class _CupyDevice:
  def __init__(self, i):
    self.id = i


def test_device_actions_validated():
  from safe_adaptation_gym_amd import _native as nat
  p = nat.device_pointer
  assert p(_Fake((130, 2)), (130, 2), 0) == 0x7f0000001000
  assert p(_Fake((130, 2), device=_TorchDevice(1)), (130, 2), 1) == 0x7f0000001000
  assert p(_Fake((130, 2), strides=(8, 4)), (130, 2), 0) == 0x7f0000001000
  assert p(_Fake((130, 2), typestr='<f8')) == 0x7f0000001000         # without a shape: a pointer, nothing asserted
  with pytest.raises(ValueError, match='float32'):
    p(_Fake((130, 2), typestr='<f8'), (130, 2), 0)
  with pytest.raises(ValueError, match='float32'):
    p(_Fake((130, 2), typestr='<f2'), (130, 2), 0)
  with pytest.raises(ValueError, match='float32'):
    p(_Fake((130, 2), typestr='>f4'), (130, 2), 0)
  for shape in ((129, 2), (131, 2), (260,), (130, 12), (1, 130, 2)):
    with pytest.raises(ValueError, match='shape'):
      p(_Fake(shape), (130, 2), 0)
  with pytest.raises(ValueError, match='contiguous'):
    p(_Fake((130, 2), strides=(16, 4)), (130, 2), 0)
  with pytest.raises(ValueError, match='device 1'):
    p(_Fake((130, 2), device=_TorchDevice(1)), (130, 2), 0)
  with pytest.raises(ValueError, match='device 3'):
    p(_Fake((130, 2), device=_CupyDevice(3)), (130, 2), 0)
  with pytest.raises(TypeError):
    p(np.zeros((130, 2), np.float32), (130, 2), 0)


def test_device_array_actions_validated():
  from safe_adaptation_gym_amd import _native as nat

  class Ctx:
    device = 0

  A = nat.DeviceArray
  assert nat.device_pointer(A(Ctx(), 4096, (64, 12), np.float32), (64, 12), 0) == 4096
  with pytest.raises(ValueError, match='float32'):
    nat.device_pointer(A(Ctx(), 4096, (64, 12), np.float64), (64, 12), 0)
  with pytest.raises(ValueError, match='shape'):
    nat.device_pointer(A(Ctx(), 4096, (64, 2), np.float32), (64, 12), 0)
  with pytest.raises(ValueError, match='contiguous'):
    nat.device_pointer(A(Ctx(), 4096, (64,), np.float32, strides=(8,)), (64,), 0)
  with pytest.raises(ValueError, match='device 0'):
    nat.device_pointer(A(Ctx(), 4096, (64, 12), np.float32), (64, 12), 1)

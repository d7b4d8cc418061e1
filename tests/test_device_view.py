"""The Python layer's one reader of device arrays (_native.device_view) under every entry point's own rule, the one owner of
device allocations (_native.DeviceBuffers) against a context that records its calls, and the signature table.  No GPU, no
library: the arrays are objects that export the CUDA array interface as a torch / cupy array does, the rules are called
through stand-ins for `self`.

Every table row is (name, array factory, what the rule returns | the exception it raises).  The rows were derived from the
rules as they stood before device_view existed - each its own parser - and checked against that code: same verdict and same
exception type for every row.  The device-1 rows of test_rule_refuses_another_device are the one deliberate difference: an array that names another GPU than
the context's was accepted by every rule but device_pointer's and is now a ValueError everywhere."""
import ctypes as C
import gc
import types

import numpy as np
import pytest

from safe_adaptation_gym_amd import _native as nat
from safe_adaptation_gym_amd.policy import MLPPolicy
from safe_adaptation_gym_amd.rollout_buffer import RolloutBuffer

BASE = 0x7f0000001000   # 4096-byte aligned
OD, NU = 8, 2           # observation rows of 32 bytes


class _Fake:
  """An object that exports __cuda_array_interface__ (as a torch / cupy array does), optionally with a .device."""

  def __init__(self, shape, typestr='<f4', strides=None, device=None, ptr=BASE):
    self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (ptr, False), 'version': 2, 'strides': strides}
    if device is not None:
      self.device = device


class _TorchDevice:
  def __init__(self, index):
    self.type, self.index = 'cuda', index


class _CupyDevice:
  def __init__(self, i):
    self.id = i


class _Ctx:
  def __init__(self, device):
    self.device = device


def _array(shape, typestr='<f4', strides=None, ptr=BASE, ctx=None):
  """The same array as a DeviceArray (of a context that names no device unless one is given)."""
  return nat.DeviceArray(ctx or object(), ptr, shape, np.dtype(typestr), strides=strides, base=(ptr, shape))


F, A = _Fake, _array
V, T = ValueError, TypeError
HOST = np.zeros((3, OD), np.float32)

# MLPPolicy.forward's observations: [rows, OD] float32, rows contiguous, 16-byte aligned, a multiple of 16 bytes apart
# -> (pointer, rows, pitch in floats)
ROWS = [
    ('no strides', lambda: F((3, OD)), (BASE, 3, OD)),
    ('dense strides', lambda: F((3, OD), strides=(32, 4)), (BASE, 3, OD)),
    ('DeviceArray, no strides', lambda: A((3, OD)), (BASE, 3, OD)),
    ('DeviceArray, pitched', lambda: A((3, OD), strides=(48, 4)), (BASE, 3, 12)),
    ('pitch 48: a larger multiple of 16', lambda: F((3, OD), strides=(48, 4)), (BASE, 3, 12)),
    ('pitch 40: no multiple of 16', lambda: F((3, OD), strides=(40, 4)), V),
    ('pitch 16: rows overlap', lambda: F((3, OD), strides=(16, 4)), V),
    ('elements 8 bytes apart', lambda: F((3, OD), strides=(64, 8)), V),
    ('pointer off 16 by 4', lambda: F((3, OD), ptr=BASE + 4), V),
    ('pointer off 16 by 8', lambda: A((3, OD), ptr=BASE + 8), V),
    ('one row', lambda: F((1, OD)), (BASE, 1, OD)),
    ('no rows', lambda: F((0, OD)), (BASE, 0, OD)),
    ('float64', lambda: F((3, OD), '<f8'), V),
    ('big-endian float32', lambda: F((3, OD), '>f4'), V),
    ('int32', lambda: A((3, OD), '<i4'), V),
    ('a row short', lambda: F((3, OD - 1)), V),
    ('1-D', lambda: F((3 * OD,)), V),
    ('3-D', lambda: F((1, 3, OD)), V),
    ('host array', lambda: HOST, T),
    ('None', lambda: None, T),
]

# MLPPolicy.backward's inputs (and update_obs_stats', PPOLearner._prepare's): time-major [planes, rows] + tail float32, rows
# contiguous, planes a whole number of rows apart and not overlapping -> (pointer, planes, rows, pitch in rows)
PLANES_SCALAR = [   # tail ()
    ('no strides', lambda: F((2, 3)), (BASE, 2, 3, 3)),
    ('dense strides: 3 rows', lambda: F((2, 3), strides=(12, 4)), (BASE, 2, 3, 3)),
    ('4 rows apart', lambda: F((2, 3), strides=(16, 4)), (BASE, 2, 3, 4)),
    ('DeviceArray, 4 rows apart', lambda: A((2, 3), strides=(16, 4)), (BASE, 2, 3, 4)),
    ('2 rows apart: planes overlap', lambda: F((2, 3), strides=(8, 4)), V),
    ('3.5 rows apart', lambda: F((2, 3), strides=(14, 4)), V),
    ('rows 8 bytes apart', lambda: F((2, 3), strides=(24, 8)), V),
    ('pointer off 16', lambda: F((2, 3), ptr=BASE + 4), (BASE + 4, 2, 3, 3)),   # (backward checks obs alone, itself)
    ('a tail where none belongs', lambda: F((2, 3, 1)), V),
    ('1-D', lambda: F((6,)), V),
    ('float64', lambda: F((2, 3), '<f8'), V),
    ('big-endian float32', lambda: F((2, 3), '>f4'), V),
    ('host array', lambda: np.zeros((2, 3), np.float32), T),
]
PLANES_OBS = [   # tail (OD,)
    ('no strides', lambda: F((2, 3, OD)), (BASE, 2, 3, 3)),
    ('dense strides', lambda: A((2, 3, OD), strides=(96, 32, 4)), (BASE, 2, 3, 3)),
    ('4 rows apart', lambda: F((2, 3, OD), strides=(128, 32, 4)), (BASE, 2, 3, 4)),
    ('2 rows apart: planes overlap', lambda: F((2, 3, OD), strides=(64, 32, 4)), V),
    ('3.5 rows apart', lambda: F((2, 3, OD), strides=(112, 32, 4)), V),
    ('pitched rows', lambda: F((2, 3, OD), strides=(192, 64, 4)), V),
    ('elements 8 bytes apart', lambda: F((2, 3, OD), strides=(192, 64, 8)), V),
    ('tail mismatch', lambda: F((2, 3, OD - 1)), V),
    ('no tail', lambda: F((2, 3)), V),
    ('float64', lambda: A((2, 3, OD), '<f8'), V),
    ('big-endian float32', lambda: F((2, 3, OD), '>f4'), V),
]

# MLPPolicy.backward's row list: contiguous int32 [count >= 1], 4-byte aligned, or (pointer, count) -> (pointer, count)
ROW_LIST = [
    ('int32 1-D', lambda: F((5,), '<i4'), (BASE, 5)),
    ('int32, dense strides', lambda: F((5,), '<i4', strides=(4,)), (BASE, 5)),
    ('DeviceArray', lambda: A((5,), '<i4'), (BASE, 5)),
    ('every other entry', lambda: F((5,), '<i4', strides=(8,)), V),
    ('int64', lambda: F((5,), '<i8'), V),
    ('float32', lambda: F((5,), '<f4'), V),
    ('2-D', lambda: F((5, 1), '<i4'), V),
    ('empty', lambda: F((0,), '<i4'), V),
    ('pointer off 4', lambda: F((5,), '<i4', ptr=BASE + 2), V),
    ('pair of int', lambda: (BASE, 5), (BASE, 5)),
    ('pair of c_void_p', lambda: (C.c_void_p(BASE), 5), (BASE, 5)),
    ('pair, no entries', lambda: (BASE, 0), V),
    ('pair, pointer off 4', lambda: (BASE + 1, 5), V),
    ('host array', lambda: np.zeros(5, np.int32), T),
]

# RolloutBuffer.advantages' device values: float32 [rows, N] with exactly the buffer's strides (P * 4, 4) -> the pointer
N_, P_ = 3, 256
VALUES = [
    ("the buffer's pitch", lambda: F((5, N_), strides=(P_ * 4, 4)), BASE),
    ("DeviceArray, the buffer's pitch", lambda: A((5, N_), strides=(P_ * 4, 4)), BASE),
    ('no strides, N != P', lambda: F((5, N_)), V),
    ('dense strides, N != P', lambda: F((5, N_), strides=(N_ * 4, 4)), V),
    ('another pitch', lambda: F((5, N_), strides=(P_ * 8, 4)), V),
    ('a plane short', lambda: F((4, N_), strides=(P_ * 4, 4)), V),
    ('float64', lambda: F((5, N_), '<f8', strides=(P_ * 4, 4)), V),
    ('big-endian float32', lambda: F((5, N_), '>f4', strides=(P_ * 4, 4)), V),
    ('pointer off 4', lambda: F((5, N_), strides=(P_ * 4, 4), ptr=BASE + 2), V),
]
VALUES_FULL = [   # N == P: the dense array has the buffer's pitch
    ('no strides, N == P', lambda: F((5, P_)), BASE),
    ('dense strides, N == P', lambda: A((5, P_), strides=(P_ * 4, 4)), BASE),
]

# device_pointer(x, shape, device, dtype): what envs.step / reset / fork, MLPPolicy's outputs, RolloutBuffer's final values and
# the planner's mask ask -> the pointer.  (tests/test_throughput_rng.py has the action rows.)
POINTER = [
    ('mask bytes', lambda: F((4,), '|u1'), ((4,), 0, np.uint8), BASE),
    ('float32 for a mask', lambda: F((4,)), ((4,), 0, np.uint8), V),
    ('int32 source indices', lambda: A((4,), '<i4'), ((4,), 0, np.int32), BASE),
    ('dense strides given', lambda: A((4, 2), strides=(8, 4)), ((4, 2), 0), BASE),
    ('a strided column', lambda: A((4,), strides=(8,)), ((4,), 0), V),
    ('a strided column, no shape asked', lambda: A((4,), strides=(8,)), (), V),
    ('no shape asked: the pointer alone', lambda: F((4,), '<f8', device=_TorchDevice(1)), (None, 0), BASE),
    ('host array', lambda: HOST, ((3, OD), 0), T),
]


def _wrong_device(kw):
  """-> [(name, factory)]: one array under torch's, cupy's and a DeviceArray's way of naming device 1, and what must pass on a
  context on device 0: device 0 named each way, a torch device without an index, a context that names none."""
  ptr, shape, typestr, strides = kw['ptr'], kw['shape'], kw.get('typestr', '<f4'), kw.get('strides')
  f = lambda dev: (lambda: F(shape, typestr, strides, dev, ptr))   # noqa: E731
  a = lambda ctx: (lambda: A(shape, typestr, strides, ptr, ctx))   # noqa: E731
  wrong = [('torch, device 1', f(_TorchDevice(1))), ('cupy, device 1', f(_CupyDevice(1))), ('DeviceArray, device 1', a(_Ctx(1)))]
  right = [('torch, device 0', f(_TorchDevice(0))), ('cupy, device 0', f(_CupyDevice(0))), ('DeviceArray, device 0', a(_Ctx(0))),
           ('torch, no index', f(_TorchDevice(None))), ('no device named', f(None)), ('DeviceArray, no device named', a(None))]
  return wrong, right


pi = types.SimpleNamespace(obs_dim=OD, nu=NU, _ctx=_Ctx(0))
buf = types.SimpleNamespace(N=N_, P=P_, _ctx=_Ctx(0))
full = types.SimpleNamespace(N=P_, P=P_, _ctx=_Ctx(0))
value = lambda p: p.value   # noqa: E731

# rule name -> (the rule as a function of the array, its table, one accepted array's arguments for the device rows)
RULES = {
    'rows': (lambda x: MLPPolicy._rows(pi, x), ROWS, dict(ptr=BASE, shape=(3, OD))),
    'planes': (lambda x: MLPPolicy._planes(pi, x, (), 'adv'), PLANES_SCALAR, dict(ptr=BASE, shape=(2, 3), strides=(16, 4))),
    'planes of observations': (lambda x: MLPPolicy._planes(pi, x, (OD,), 'obs'), PLANES_OBS, dict(ptr=BASE, shape=(2, 3, OD))),
    'row list': (lambda x: MLPPolicy._row_list(pi, x), ROW_LIST, dict(ptr=BASE, shape=(5,), typestr='<i4')),
    'values': (lambda x: value(RolloutBuffer._values(buf, 'value', x, 5, 'value')), VALUES, dict(ptr=BASE, shape=(5, N_), strides=(P_ * 4, 4))),
    'values, N == P': (lambda x: value(RolloutBuffer._values(full, 'value', x, 5, 'value')), VALUES_FULL, dict(ptr=BASE, shape=(5, P_))),
}
PREFIX = {'rows': 'MLPPolicy', 'planes': 'MLPPolicy.backward: adv', 'planes of observations': 'MLPPolicy.backward: obs',
          'row list': 'MLPPolicy.backward: rows', 'values': 'RolloutBuffer.advantages', 'values, N == P': 'RolloutBuffer.advantages'}


@pytest.mark.parametrize('rule', list(RULES))
def test_rule_table(rule):
  fn, table, _ = RULES[rule]
  for name, make, want in table:
    if isinstance(want, type):
      with pytest.raises(want) as e:
        fn(make())
      assert str(e.value).startswith(PREFIX[rule]), (rule, name, str(e.value))
    else:
      assert fn(make()) == want, (rule, name)


@pytest.mark.parametrize('rule', list(RULES))
def test_rule_refuses_another_device(rule):
  fn, table, accepted = RULES[rule]
  wrong, right = _wrong_device(accepted)
  want = fn(F(accepted['shape'], accepted.get('typestr', '<f4'), accepted.get('strides'), None, accepted['ptr']))
  for name, make in right:
    assert fn(make()) == want, (rule, name)
  for name, make in wrong:
    with pytest.raises(ValueError, match='device 1') as e:
      fn(make())
    assert str(e.value).startswith(PREFIX[rule]), (rule, name, str(e.value))


def test_device_pointer_table():
  for name, make, args, want in POINTER:
    if isinstance(want, type):
      with pytest.raises(want):
        nat.device_pointer(make(), *args)
    else:
      assert nat.device_pointer(make(), *args) == want, name
  for dev in (_TorchDevice(1), _CupyDevice(1)):
    with pytest.raises(ValueError, match='device 1'):
      nat.device_pointer(F((4,), '|u1', device=dev), (4,), 0, np.uint8)
    assert nat.device_pointer(F((4,), '|u1', device=dev), (4,), 1, np.uint8) == BASE
    assert nat.device_pointer(F((4,), '|u1', device=dev), (4,), None, np.uint8) == BASE


def test_policy_outputs_need_no_rewrap():
  """An output view that spells out its dense strides (a plane of a time-major array) is contiguous as it stands."""
  out = lambda x, shape: MLPPolicy._out(pi, x, shape, 'value')   # noqa: E731
  assert out(None, (3,)) is None
  assert out(A((3,), strides=(4,)), (3,)) == BASE and out(F((3, NU), strides=(8, 4)), (3, NU)) == BASE
  for bad, word in ((A((3,), strides=(8,)), 'contiguous'), (A((4,)), 'shape'), (A((3,), '<f8'), 'float32'),
                    (A((3,), ctx=_Ctx(1)), 'device 1')):
    with pytest.raises(ValueError, match=word) as e:
      out(bad, (3,))
    assert str(e.value).startswith('MLPPolicy: value: ')


def test_device_view_record():
  v = nat.device_view(F((2, 3), '<f8', device=_CupyDevice(2)))
  assert v == (BASE, (2, 3), (24, 8), np.dtype('<f8'), 2) and v.contiguous
  assert nat.device_view(F((2, 3), '<f8', strides=(24, 8))) == nat.device_view(F((2, 3), '<f8'))   # strides are always concrete
  w = nat.device_view(A((2, 3), '<u1', strides=(256, 1), ctx=_Ctx(1)))
  assert (w.ptr, w.shape, w.strides, w.dtype, w.device) == (BASE, (2, 3), (256, 1), np.dtype('u1'), 1) and not w.contiguous
  assert nat.device_view(A((2,))).device is None and nat.device_view(F((2,), device=_TorchDevice(None))).device is None
  assert nat.device_view(F((2,), device=_TorchDevice(1)), 'x', device=1).device == 1
  with pytest.raises(ValueError, match='^actions on device 1: .* device 0'):
    nat.device_view(F((2,), device=_TorchDevice(1)), 'actions', device=0)
  with pytest.raises(TypeError, match='^actions: ndarray is not a device array'):
    nat.device_view(HOST, 'actions')
  assert nat.is_device_array(F((2,))) and nat.is_device_array(A((2,))) and not nat.is_device_array(HOST) and not nat.is_device_array(None)


def test_dense_strides_are_numpys():
  for dtype in ('u1', '<f4', '<f8'):
    for shape in ((), (5,), (2, 3), (2, 3, 8), (1, 1), (4, 1, 3)):
      assert nat.dense_strides(shape, dtype) == np.zeros(shape, dtype).strides, (shape, dtype)
  # an empty array keeps the strides of its rows (NumPy gives it zeros, or these, depending on its version)
  assert nat.dense_strides((0, 8), '<f4') == (32, 4) and nat.dense_strides((2, 0), '<f4') == (4, 4) and nat.dense_strides((0,), 'u1') == (1,)


# ------------------------------------------------------------------------------------------------------------------
# DeviceBuffers
# ------------------------------------------------------------------------------------------------------------------
class _Recorder:
  """A context that records dev_alloc / dev_free / dev_upload; alloc number fail_at raises."""

  def __init__(self, fail_at=None):
    self.h, self.fail_at, self.allocated, self.freed, self.uploads = C.c_void_p(1), fail_at, [], [], []

  def dev_alloc(self, nbytes):
    if len(self.allocated) == self.fail_at:
      raise nat.SagError('sag_dev_alloc failed')
    self.allocated.append(0x1000 * (len(self.allocated) + 1))
    return C.c_void_p(self.allocated[-1])

  def dev_free(self, p):
    self.freed.append(p.value)

  def dev_upload(self, dst, arr):
    self.uploads.append((dst.value, arr.nbytes, bool(np.asarray(arr).any())))


def test_device_buffers_free_each_allocation_once():
  c = _Recorder()
  b = nat.DeviceBuffers(c)
  p = b.alloc('mean', 64)
  q = b.alloc('words', 80, zero=True)
  assert isinstance(p, C.c_void_p) and b['mean'] is p and b.get('words') is q and b.get('budget') is None
  assert 'mean' in b and 'budget' not in b and c.uploads == [(q.value, 80, False)]
  with pytest.raises(KeyError):
    b['budget']
  with pytest.raises(KeyError):
    b.alloc('mean', 8)                      # a name is taken once: nothing is allocated over it
  assert len(c.allocated) == 2
  b.close()
  assert sorted(c.freed) == sorted(c.allocated) and 'mean' not in b
  b.close()                                 # a second close does nothing
  del b
  gc.collect()                              # nor does collection after close
  assert sorted(c.freed) == sorted(c.allocated) and len(c.freed) == 2


def test_device_buffers_after_the_context_is_destroyed():
  c = _Recorder()
  b = nat.DeviceBuffers(c)
  b.alloc('a', 8), b.alloc('b', 8)
  c.h = None                                # Context.close(): no handle is left to free through
  b.close()
  del b
  gc.collect()
  assert c.freed == []


def test_device_buffers_failed_alloc_and_collection():
  c = _Recorder(fail_at=2)
  b = nat.DeviceBuffers(c)
  b.alloc('a', 8), b.alloc('b', 8)
  with pytest.raises(nat.SagError):
    b.alloc('c', 8)
  assert 'c' not in b
  del b                                     # no close(): collection frees the two that exist, once
  gc.collect()
  assert sorted(c.freed) == sorted(c.allocated) and len(c.freed) == 2


def test_owners_close_through_their_buffers():
  """close() of a policy / learner / buffer is a close of its owner; the handles the tests read go back to None."""
  from safe_adaptation_gym_amd.learner import PPOLearner
  c = _Recorder()
  own = nat.DeviceBuffers(c)
  learner = PPOLearner.__new__(PPOLearner)
  learner._own, learner._ctx = own, c
  learner._m, learner._v = own.alloc('m', 8), own.alloc('v', 8)
  learner.close()
  learner.close()
  assert sorted(c.freed) == sorted(c.allocated) and learner._m is None and learner._v is None and learner._index is None
  own = nat.DeviceBuffers(c)
  pol = MLPPolicy.__new__(MLPPolicy)
  pol._own, pol._buf = own, own.alloc('params', 8)
  pol.close()
  pol.close()
  assert sorted(c.freed) == sorted(c.allocated) and pol._buf is None and pol._obs_table is None


# ------------------------------------------------------------------------------------------------------------------
# the signature table
# ------------------------------------------------------------------------------------------------------------------
def test_signature_table():
  assert nat.EXPORTS == list(nat.SIGNATURES) and len(set(nat.EXPORTS)) == len(nat.EXPORTS)
  for name, (argtypes, restype) in nat.SIGNATURES.items():
    assert isinstance(argtypes, list), name
    C.CFUNCTYPE(restype, *argtypes)         # ctypes itself refuses what is no argument or result type
  assert nat.SIGNATURES['sag_last_error'][1] is C.c_char_p and nat.SIGNATURES['sag_task_desc_check'][1] is C.c_char_p
  assert nat.SIGNATURES['sag_world_config_default'][1] is None and nat.SIGNATURES['sag_device_count'] == ([], C.c_int)


def test_load_applies_the_table_to_every_symbol():
  lib = nat.load()
  for name, (argtypes, restype) in nat.SIGNATURES.items():
    fn = getattr(lib, name)
    assert list(fn.argtypes) == argtypes and fn.restype is restype, name

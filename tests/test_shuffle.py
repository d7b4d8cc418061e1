"""sag_permutation_device (csrc/sag_shuffle.hpp) against the NumPy restatement of tests/shuffle_ref.py, bit for bit: even and
odd widths of the walk domain, a size just past a power of two (the longest walks) and an exact power (no walk).  Guard words
behind the array, the draw and the key, repeatability, the refusals.  The cases of n <= 4097 also run on the host build of the
device sources (test_shuffle_hostemu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import shuffle_ref as S
from test_device_reset import KEY

HOSTEMU = bool(os.environ.get('SAG_HOSTEMU'))
ERR_ARG = -1
GUARD = 16
SENTINEL = -77
SIZES = [1, 2, 33, 130, 4097] + ([] if HOSTEMU else [65537, 2**20])


@pytest.fixture(scope='module')
def nat():
  from safe_adaptation_gym_amd import _native
  if _native.device_count() < 1:
    pytest.fail('no HIP device visible: the GPU tests need an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(nat):
  c = nat.Context('point', 8, seed=KEY)
  yield c
  c.close()


def _run(c, n, draw, offset=0):
  """The n entries and the GUARD words behind them, written at `offset` words into an array filled with SENTINEL."""
  d = c.dev_alloc((offset + n + GUARD) * 4)
  c.dev_upload(d, np.full(offset + n + GUARD, SENTINEL, np.int32))
  c.permutation(n, draw, d.value + 4 * offset)
  c.wait()
  w = c.dev_download(d, (offset + n + GUARD,), np.int32)
  c.dev_free(d)
  assert (w[:offset] == SENTINEL).all(), 'a write ahead of d_index'
  assert (w[offset + n:] == SENTINEL).all(), 'a write behind d_index + n'
  return w[offset:offset + n]


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_permutation_equals_the_restatement_bit_for_bit(ctx, n):
  for draw in (0, 0xfffffffe):
    got = _run(ctx, n, draw)
    want = S.permutation(n, draw, KEY)
    assert got.tobytes() == want.tobytes(), (n, draw, np.flatnonzero(got != want)[:8])
    assert np.array_equal(np.sort(got), np.arange(n))


@pytest.mark.gpu
def test_draw_key_repeat_and_an_odd_word_offset(ctx):
  n = 4097
  a, b = _run(ctx, n, 3), _run(ctx, n, 4)
  assert np.count_nonzero(a == b) < n // 100, 'two draws agree'
  assert _run(ctx, n, 3).tobytes() == a.tobytes(), 'the same call twice'
  assert _run(ctx, n, 3, offset=3).tobytes() == a.tobytes(), 'd_index at a 4-byte, not 16-byte, boundary'
  ctx.set_seed(KEY ^ 0x100000001)
  try:
    c = _run(ctx, n, 3)
    assert c.tobytes() == S.permutation(n, 3, KEY ^ 0x100000001).tobytes() and np.count_nonzero(a == c) < n // 100
  finally:
    ctx.set_seed(KEY)


@pytest.mark.gpu
def test_refusals_enqueue_nothing(ctx):
  c = ctx
  d = c.dev_alloc(64 * 4)
  c.dev_upload(d, np.full(64, SENTINEL, np.int32))
  f = c.lib.sag_permutation_device
  assert f(None, 8, 0, d) == ERR_ARG
  assert f(c.h, 8, 0, None) == ERR_ARG
  assert f(c.h, 8, 0, C.c_void_p(d.value + 2)) == ERR_ARG
  assert f(c.h, 0, 0, d) == ERR_ARG and f(c.h, -5, 0, d) == ERR_ARG
  assert b'sag_permutation_device' in c.lib.sag_last_error(c.h)
  c.wait()
  assert (c.dev_download(d, (64,), np.int32) == SENTINEL).all()
  c.dev_free(d)

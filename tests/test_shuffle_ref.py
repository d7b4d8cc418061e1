"""tests/shuffle_ref.py pinned on its own (no GPU): the restatement of sag_permutation_device's pi is a bijection at every
size class, changes with the draw, and over many draws fills the position x value table evenly.  The bounds are the
statistics' own: |z| of 130^2 cells stays below 6 (P(|z| > 6) ~ 2e-9 per cell), and chi^2 / dof of a chi^2 with 129^2 degrees
of freedom has standard deviation sqrt(2 / 129^2) = 0.011 - five of them are 0.055."""
import numpy as np
import pytest

import shuffle_ref as S

KEY = 0x1234567800000abc   # test_device_reset.KEY: a key whose high word is not zero


@pytest.mark.parametrize('n', [1, 2, 3, 5, 31, 33, 130, 1000, 4097, 65537])
def test_bijection(n):
  for draw in (0, 7, 0xffffffff):
    walks = []
    p = S.permutation(n, draw, KEY, walks=walks)
    assert p.dtype == np.int32 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n)), (n, draw)
    assert walks[0] <= 64, walks   # 2^b < 2 n: a walk of k rounds has probability below 2^-(k - 1) per element


def test_bits_and_widths():
  assert [S.bits(n) for n in (1, 2, 3, 4, 5, 8, 9, 4096, 4097, 65536, 65537, 2**20, 2**31 - 1)] == [2, 2, 2, 2, 3, 3, 4, 12, 13, 16, 17, 20, 31]
  for b in (2, 3, 12, 17):   # F permutes [0, 2^b), even and odd b
    f = S.feistel(np.arange(1 << b), b, 3, KEY)
    assert np.array_equal(np.sort(f), np.arange(1 << b))


def test_an_exact_power_of_two_needs_no_walk():
  walks = []
  S.permutation(4096, 5, KEY, walks=walks)
  assert walks == [1]


def test_two_draws_agree_in_fewer_than_one_percent_of_positions():
  a, b = S.permutation(4096, 0, KEY), S.permutation(4096, 1, KEY)
  same = np.count_nonzero(a == b)
  print(f'{same} of 4096 positions agree')
  assert same < 41
  assert np.array_equal(a, S.permutation(4096, 0, KEY))                       # the same call, the same array
  assert np.count_nonzero(a == S.permutation(4096, 0, KEY ^ 1)) < 41          # the key matters too


def test_position_value_table_is_flat_over_16384_draws():
  z, chi = S.flatness(S.table(130, np.arange(16384), KEY))
  print(f'n = 130, 16384 draws: max |z| = {z:.2f}, chi^2 / dof = {chi:.4f}')
  assert z <= 6.0
  assert abs(chi - 1.0) <= 0.055

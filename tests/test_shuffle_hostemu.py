"""The device permutation and the backward pass over a row list without a GPU, two ways (tests/hostemu: the library's own device
sources compiled for the host; csrc/sag_shuffle.hpp and the ROWS instances of csrc/sag_policy_grad.hpp keep every index, LDS
word and address of the device):
  * the small cases of test_shuffle.py (n <= 4097) and test_policy_grad_rows.py (planes of <= 130 rows, hidden <= 96) in a child
    process against the unsanitized clang host build, selected through SAG_LIB + SAG_HOSTEMU=1 the way
    test_policy_grad_hostemu.py does (its own tag keeps the library apart from the other builds);
  * a stand-alone program (tests/hostemu/shuffle_main.cpp) compiled with AddressSanitizer and UndefinedBehaviorSanitizer and
    linked against the sanitized host build: the permutation at n = 1, 33 and 4097 into an array that ends its allocation, the
    rows backward with lists of 1, 33 and 97 entries - out-of-range ones among them - over planes whose last row ends the
    allocation, compared with plain double-precision loops.  The executable runs on its own; no sanitized code is loaded into
    python."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTEMU = os.path.join(ROOT, 'tests', 'hostemu')
sys.path.insert(0, HOSTEMU)


def test_kernel_cases_on_the_emulated_device():
  import build as hb   # tests/hostemu/build.py
  if not os.path.exists(hb.CLANG):
    pytest.skip('no clang for the host build')
  lib = hb.build('clang', False, False, (), False, False, 'shuffle')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_shuffle.py'),
                      os.path.join(ROOT, 'tests', 'test_policy_grad_rows.py'), '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                     capture_output=True, text=True, timeout=1500)
  tail = r.stdout[-1500:] + r.stderr[-1500:]
  assert r.returncode == 0, tail
  m = re.search(r'(\d+) passed', r.stdout)
  # the permutation: 5 sizes, the draws, the refusals; the rows backward: 11 cases, 2 of the identity, table, accumulate, refusals
  assert m and int(m.group(1)) >= 23 and 'skipped' not in r.stdout.splitlines()[-1], tail
  # the library exports what the package binds
  from safe_adaptation_gym_amd import _native
  import ctypes
  host = ctypes.CDLL(lib)
  assert all(hasattr(host, s) for s in ('sag_permutation_device', 'sag_policy_backward_rows_device')) and \
      {'sag_permutation_device', 'sag_policy_backward_rows_device'} <= set(_native.EXPORTS)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
  if not shutil.which('g++'):
    pytest.skip('no g++ for the sanitizer build')
  import build as hb
  lib = hb.build('gcc')   # -fsanitize=address,undefined
  exe = str(tmp_path / 'shuffle_main')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-ffp-contract=off',
                         '-I', os.path.join(ROOT, 'include'), os.path.join(HOSTEMU, 'shuffle_main.cpp'), lib,
                         '-Wl,-rpath,' + os.path.dirname(lib), '-o', exe])
  env = dict(os.environ, SAG_HOSTEMU='1', ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
  assert 'shuffle_main: ok' in r.stdout, r.stdout[-2000:]

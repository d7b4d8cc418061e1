"""Observation normalisation without a GPU, two ways (tests/hostemu: the library's own device sources compiled for the host;
csrc/sag_obs_norm.hpp keeps every index and LDS word of the device, and the NORM instances of the policy kernels are the
device's staging loops):
  * the statistics, forward, backward and refusal cases of test_obs_norm.py (hidden <= 64 forward, 32 backward) in a child
    process against the unsanitized clang host build, selected through SAG_LIB + SAG_HOSTEMU=1 the way
    test_learner_kernels_hostemu.py does (its own tag keeps the library apart from the other builds);
  * a stand-alone program (tests/hostemu/obs_norm_main.cpp) compiled with AddressSanitizer and UndefinedBehaviorSanitizer and
    linked against the sanitized host build: the three functions on each robot, exact-size inputs whose last counted row ends
    the allocation, guard words behind the state, the table and every output.  The executable runs on its own; no sanitized
    code is loaded into python."""
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
  lib = hb.build('clang', False, False, (), False, False, 'obs_norm')
  env = dict(os.environ, SAG_LIB=lib, SAG_HOSTEMU='1', PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, 'tests'))
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_obs_norm.py'), '-m', 'gpu', '-q', '-x',
                      '-p', 'no:cacheprovider', '-k', 'stats or forward or backward or refusals'], cwd=ROOT, env=env, capture_output=True,
                     text=True, timeout=900)
  tail = r.stdout[-1500:] + r.stderr[-1500:]
  assert r.returncode == 0, tail
  m = re.search(r'(\d+) passed', r.stdout)
  # 12 + 3 + 1 + 1 of the statistics, 12 + 1 of the forward, 6 of the backward, the refusals
  assert m and int(m.group(1)) >= 37 and 'skipped' not in r.stdout.splitlines()[-1], tail
  # the library exports what the package binds (sag_obs_stats_device and the two _norm entry points among them)
  from safe_adaptation_gym_amd import _native
  import ctypes
  host = ctypes.CDLL(lib)
  assert all(hasattr(host, s) for s in _native.EXPORTS if 'obs_stats' in s or '_norm_' in s)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
  if not shutil.which('g++'):
    pytest.skip('no g++ for the sanitizer build')
  import build as hb
  lib = hb.build('gcc')   # -fsanitize=address,undefined
  exe = str(tmp_path / 'obs_norm_main')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-ffp-contract=off',
                         '-I', os.path.join(ROOT, 'include'), os.path.join(HOSTEMU, 'obs_norm_main.cpp'), lib,
                         '-Wl,-rpath,' + os.path.dirname(lib), '-o', exe])
  env = dict(os.environ, SAG_HOSTEMU='1', ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
  assert 'obs_norm_main: ok' in r.stdout, r.stdout[-2000:]

"""CPU: the range rule of rsl::launch (csrc/rsl_launch_limits.h) in a stand-alone program, g++ alone and under the
undefined-behaviour and address sanitizers: which block counts, grid heights and thread counts a launch accepts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'radar-slam_amd', 'csrc')

CXX_SRC = r'''
#include <cstdio>
#include "rsl_launch_limits.h"
int main() {
  using rsl::launch_in_range;
  const long long gx[] = {0, 1, (1LL << 31) - 1, 1LL << 31, (1LL << 32) + 1, -1, -(1LL << 32) + 1};
  const long long gy[] = {0, 1, 65535, 65536};
  const long long th[] = {0, 1, 1024, 1025};
  for (long long v : gx) std::printf("gx %lld %d\n", v, (int)launch_in_range(v, 1, 256));
  for (long long v : gy) std::printf("gy %lld %d\n", v, (int)launch_in_range(1, v, 256));
  for (long long v : th) std::printf("threads %lld %d\n", v, (int)launch_in_range(1, 1, v));
  return 0;
}
'''

EXPECT = {
    'gx': {0: 0, 1: 1, 2 ** 31 - 1: 1, 2 ** 31: 0, 2 ** 32 + 1: 0, -1: 0, -2 ** 32 + 1: 0},
    'gy': {0: 0, 1: 1, 65535: 1, 65536: 0},
    'threads': {0: 0, 1: 1, 1024: 1, 1025: 0},
}


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_launch_range_rule(tmp_path):
    src = tmp_path / 'limits.cpp'
    src.write_text(CXX_SRC)
    exe = tmp_path / 'limits'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-fsanitize=undefined,address',
                    '-fno-sanitize-recover=all', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {k: {} for k in EXPECT}
    for line in out.strip().splitlines():
        what, v, ok = line.split()
        got[what][int(v)] = int(ok)
    assert got == EXPECT

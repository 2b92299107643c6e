"""How the stand-alone sanitizer programs under tools/probes are compiled: one place for the tests that run them."""
import os
import shutil

SANITIZER_FLAGS = ['-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-pthread']


def compile_command(src, exe):
  """host compiler + flags that link the sanitizer runtimes STATICALLY: the program then starts in whatever environment
  the suite runs in, and the test leaves that environment alone"""
  for name in ('c++', 'g++'):
    cxx = shutil.which(name)
    if cxx and 'clang' not in os.path.realpath(cxx):
      return [cxx] + SANITIZER_FLAGS + ['-static-libasan', '-static-libubsan', src, '-o', exe]
  for cxx in (shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
    if cxx and os.path.exists(cxx):
      return [cxx] + SANITIZER_FLAGS + [src, '-o', exe]      # clang links its sanitizer runtimes statically by default
  raise RuntimeError('no host C++ compiler found')

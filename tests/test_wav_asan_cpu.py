"""Host AddressSanitizer + UBSan run over the native WAV reader (no GPU): csrc/io/wav_io.cpp
compiled from source with -fsanitize=address,undefined next to its stand-alone driver
tools/asan/wav_check.cpp (accepted and refused header variants, every truncation length of a
valid file, seeded single-byte mutations of the first 64 bytes, through the probe, the single
read and the threaded batch read).  Any sanitizer report or failed check fails the test."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_wav_reader_under_asan_ubsan(tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "run-wav"], env=env,
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "wav sanitizer checks: clean" in out, out[-2000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]

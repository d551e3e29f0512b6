"""tests/native/knobs_test.cpp: the table and the parser of tfidf_open's numeric environment knobs
(csrc/knobs.h) against hand-written expectations (unset, empty, both bounds and their neighbours,
hexadecimal and octal, trailing characters, a non-power-of-two for TFIDF_VCAP, 1 and 2^20 for the
megabyte budgets, the 32-bit reading of the load limits), in a stand-alone program built with
AddressSanitizer (its runtime linked into the program) and UndefinedBehaviorSanitizer.  No GPU, and
nothing of the library that Python loads runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO


def test_knob_table_and_parser_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "knobs_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-I", os.path.join(PKG, "csrc"), "-o", exe,
           os.path.join(REPO, "tests", "native", "knobs_test.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("this compiler cannot link the sanitizers: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("cases ok")

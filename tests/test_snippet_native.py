"""tests/native/snippet_host_test.c: the host half of snippets (csrc/snippet_host.c: the check and
tfidf_result_snippet) on edge inputs (an empty corpus, zero jobs, a job whose query index or
document is out of range, a document at the buffer's very end, NUL bytes) in a stand-alone program
built with AddressSanitizer (its runtime linked into the program) and UndefinedBehaviorSanitizer.
No GPU, and nothing of the library that Python loads runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO


def test_snippet_host_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "snippet_host_test")
    cmd = [cc, "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-o", exe,
           os.path.join(REPO, "tests", "native", "snippet_host_test.c"), os.path.join(PKG, "csrc", "snippet_host.c")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("this compiler cannot link the sanitizers: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")

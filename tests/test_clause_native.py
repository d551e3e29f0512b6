"""tests/native/query_ops_test.c: the operator parser of `tfidf --query FILE --query-ops`
(host/query_ops.h) on edge lines, in a stand-alone program built with AddressSanitizer (its
runtime linked into the program) and UndefinedBehaviorSanitizer; then the refusals of the CLI's
clause options that are decided before anything touches a GPU.  No GPU, and nothing of the
library that Python loads runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

import tfidf_abi
from conftest import PKG, REPO


def test_query_ops_parser_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "query_ops_test")
    cmd = [cc, "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-I", os.path.join(PKG, "host"), "-o", exe,
           os.path.join(REPO, "tests", "native", "query_ops_test.c")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("this compiler cannot link the sanitizers: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def cli(tmp_path, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=tmp_path, capture_output=True, timeout=60)


def test_cli_refuses_before_any_device_work(tmp_path):
    (tmp_path / "input").mkdir()
    (tmp_path / "input" / "doc1").write_bytes(b"a b")
    (tmp_path / "q.txt").write_bytes(b"+a b\n")
    for args, word in (
        (["--query-ops"], b"--query FILE"),
        (["--query-all"], b"--query FILE"),
        (["--min-match", "2"], b"--query FILE"),
        (["--query-ops", "--bm25"], b"--query FILE"),
        (["--query", "q.txt", "--min-match", "4096"], b"--min-match"),
        (["--query", "q.txt", "--min-match", "-1"], b"--min-match"),
        (["--query", "q.txt", "--min-match", "2x"], b"--min-match"),
        (["--query", "q.txt", "--min-match", ""], b"--min-match"),
        (["--query", "q.txt", "--min-match", "99999999999999999999"], b"--min-match"),
    ):
        p = cli(tmp_path, *args)
        assert p.returncode == 2 and word in p.stderr, (args, p.returncode, p.stderr)
    assert not (tmp_path / "output.txt").exists() and not (tmp_path / "hits.txt").exists()

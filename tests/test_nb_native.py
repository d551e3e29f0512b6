"""tests/native/nb_host_test.c: the CLI's labels-file parser (host/labels_file.h: names to classes
in byte order, bad lines refused with their number) and the host Naive Bayes functions
(csrc/nb_host.c) on edge inputs, in a stand-alone program built with AddressSanitizer (its runtime
linked into the program) and UndefinedBehaviorSanitizer; then the refusals of `tfidf --labels ..`
that are decided before anything touches a GPU.  No GPU, and nothing of the library that Python
loads runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

import tfidf_abi
from conftest import PKG, REPO


def test_labels_parser_and_nb_host_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "nb_host_test")
    cmd = [cc, "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-o", exe,
           os.path.join(REPO, "tests", "native", "nb_host_test.c"), os.path.join(PKG, "csrc", "nb_host.c"), "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("this compiler cannot link the sanitizers: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def cli(tmp_path, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=tmp_path, capture_output=True, timeout=60)


def test_cli_refuses_before_any_device_work(tmp_path):
    (tmp_path / "input").mkdir()
    (tmp_path / "input" / "doc1").write_bytes(b"a b")
    good = tmp_path / "labels.txt"
    good.write_bytes(b"doc1\tx\n")
    for args, word in (
        (["--labels", "labels.txt"], b"--classify"),                                         # neither mode
        (["--labels", "labels.txt", "--classify", "new", "--classify-unlabelled"], b"--classify"),   # both
        (["--classify-unlabelled"], b"--labels"),
        (["--classify", "new"], b"--labels"),
        (["--nb-complement"], b"--labels"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--nb-alpha", "0"], b"--nb-alpha"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--nb-alpha", "nan"], b"--nb-alpha"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--nb-alpha", "-1"], b"--nb-alpha"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--nb-alpha", "1e300"], b"--nb-alpha"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--nb-alpha", "1x"], b"--nb-alpha"),
        (["--labels", "missing.txt", "--classify-unlabelled"], b"cannot open"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--shards", "2"], b"one shard"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--gpus", "2"], b"one shard"),
        (["--labels", "labels.txt", "--classify-unlabelled", "--model", "m.bin", "--transform", "input"], b"--model"),
    ):
        p = cli(tmp_path, *args)
        assert p.returncode == 2 and word in p.stderr, (args, p.returncode, p.stderr)
    for text, word in ((b"doc1 x\n", b"line 1"), (b"doc1\tx\ndoc2\n", b"line 2"), (b"doc1\tx\n\n", b"line 2"),
                       (b"doc01\tx\n", b"line 1"), (b"", b"no line"), (b"doc1\tx\ndoc1\ty\n", b"twice"),
                       (b"".join(b"doc%d\tc%d\n" % (i + 1, i) for i in range(257)), b"classes")):
        bad = tmp_path / "bad.txt"
        bad.write_bytes(text)
        p = cli(tmp_path, "--labels", "bad.txt", "--classify-unlabelled")
        assert p.returncode == 2 and word in p.stderr, (text[:20], p.returncode, p.stderr)
    assert not (tmp_path / "output.txt").exists() and not (tmp_path / "classes.txt").exists()

"""`tfidf --query F --top 3 --snippets 8` on a golden case, alone and with --bm25, --fuzzy auto,
--query-ops and --shards 2: snippets.txt equals the lines rendered from tests/snippet_ref.py for
the hits the tool wrote, and output.txt and hits.txt are byte-identical to a run without the
option.  The combinations the tool refuses exit 2."""
import os
import shutil
import subprocess

import pytest

import match_corpus as MC
import snippet_ref as R
import tfidf_abi
from conftest import GOLDEN
from helpers import load_golden
from test_gpu_match import cli_expand

pytestmark = pytest.mark.gpu

CASE = "g5_w3"


def run_cli(cwd, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=cwd, capture_output=True, timeout=120)


@pytest.fixture(scope="module")
def case():
    g = load_golden(CASE)
    docs = {i + 1: bytes(g["data"][int(g["off"][i]):int(g["off"][i + 1])]) for i in range(len(g["off"]) - 1)}
    terms, df, _ = MC.dictionary(MC.docs_of(g["data"], g["off"]))
    pats = MC.drawn_patterns(terms, 24, seed=9)
    plain = [b" ".join(terms[(7 * i + j) % len(terms)] for j in range(3)) for i in range(8)] + [b"", b"zzabsent " + terms[0]]
    return dict(docs=docs, terms=terms, df=df, plain=plain, fuzzy=[b" ".join(pats[3 * i:3 * i + 3]) for i in range(8)])


def check(tmp_path, lines, texts, docs, *args):
    """the tool with and without --snippets over `lines`; texts: what reaches the ranking call"""
    for sub in ("with", "without"):
        os.makedirs(tmp_path / sub)
        shutil.copytree(os.path.join(GOLDEN, CASE, "input"), tmp_path / sub / "input")
        (tmp_path / sub / "q.txt").write_bytes(b"\n".join(lines) + b"\n")
    p = run_cli(tmp_path / "with", "--query", "q.txt", "--top", "3", "--snippets", "8", *args)
    assert p.returncode == 0, p.stderr
    p = run_cli(tmp_path / "without", "--query", "q.txt", "--top", "3", *args)
    assert p.returncode == 0, p.stderr
    hits = (tmp_path / "with" / "hits.txt").read_bytes()
    assert hits == (tmp_path / "without" / "hits.txt").read_bytes()
    assert (tmp_path / "with" / "output.txt").read_bytes() == (tmp_path / "without" / "output.txt").read_bytes()
    assert not (tmp_path / "without" / "snippets.txt").exists()
    jobs = [(int(f[0][1:]) - 1, int(f[1][3:])) for f in (l.split(b"\t") for l in hits.splitlines())]
    assert len(jobs) >= 6
    rows, _ = R.run(docs, texts, jobs, window=8, max_marks=32)
    want = b"".join(R.render(q + 1, d, r, len(R.query_terms(texts[q])[0])) for (q, d), r in zip(jobs, rows))
    assert (tmp_path / "with" / "snippets.txt").read_bytes() == want
    assert b"[" in want


@pytest.mark.parametrize("args", [(), ("--bm25",), ("--shards", "2"), ("--bm25", "--shards", "2")], ids=" ".join)
def test_cli_snippets(case, tmp_path, args):
    check(tmp_path, case["plain"], case["plain"], case["docs"], *args)


def test_cli_snippets_fuzzy(case, tmp_path):
    rewritten = [line for _, line in cli_expand(case["terms"], case["df"], case["fuzzy"])]
    check(tmp_path, case["fuzzy"], rewritten, case["docs"], "--fuzzy", "auto")


def test_cli_snippets_query_ops(case, tmp_path):
    t = case["terms"]
    lines = [b"+" + t[i] + b" " + t[i + 1] + b" " + t[i + 2] + b" -" + t[i + 3] for i in range(0, 40, 5)]
    texts = [t[i] + b" " + t[i + 1] + b" " + t[i + 2] for i in range(0, 40, 5)]     # must, then should; no must-not word
    check(tmp_path, lines, texts, case["docs"], "--query-ops")


def test_cli_refused_combinations(tmp_path):
    (tmp_path / "q.txt").write_bytes(b"a\n")
    for args in (("--query", "q.txt", "--snippets", "8", "--ngrams", "2"), ("--snippets", "8"),
                 ("--model", "m.bin", "--transform", "x", "--snippets", "8"), ("--query", "q.txt", "--snippets", "0"),
                 ("--query", "q.txt", "--snippets", "1025"), ("--query", "q.txt", "--snippets", "8", "--snippet-marks", "1025")):
        p = run_cli(tmp_path, *args)
        assert p.returncode == 2, (args, p.stderr)

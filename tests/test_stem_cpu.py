"""The analyzer's Porter stemmer on the host (include/tfidf.h, section "analyzer", step 3):
tests/stem_ref.py, the definition in plain Python, against the paper's own examples step by
step, and tfidf_stem_porter and tfidf_analyze_host against stem_ref.  No GPU call."""
import numpy as np
import pytest

import stem_ref
import tfidf_abi
from helpers import docs_to_arrays, windowed

PAPER = {
    "step1a": "caresses caress ponies poni ties ti caress caress cats cat",
    "step1b": "feed feed agreed agree plastered plaster bled bled motoring motor sing sing conflated conflate "
              "troubled trouble sized size hopping hop tanned tan falling fall hissing hiss fizzed fizz failing fail "
              "filing file",
    "step1c": "happy happi sky sky",
    "step2": "relational relate conditional condition rational rational valenci valence hesitanci hesitance "
             "digitizer digitize conformabli conformable radicalli radical differentli different vileli vile "
             "analogousli analogous vietnamization vietnamize predication predicate operator operate feudalism feudal "
             "decisiveness decisive hopefulness hopeful callousness callous formaliti formal sensitiviti sensitive "
             "sensibiliti sensible",
    "step3": "triplicate triplic formative form formalize formal electriciti electric electrical electric hopeful hope "
             "goodness good",
    "step4": "revival reviv allowance allow inference infer airliner airlin gyroscopic gyroscop adjustable adjust "
             "defensible defens irritant irrit replacement replac adjustment adjust dependent depend adoption adopt "
             "homologou homolog communism commun activate activ angulariti angular homologous homolog effective effect "
             "bowdlerize bowdler",
    "step5a": "probate probat rate rate cease ceas",
    "step5b": "controll control roll roll",
}
WHOLE = ("generalizations gener oscillators oscil relational relat running run agreed agre conflated conflat "
         "controlling control rolling roll abilities abil sensibilities sensibl internationalization internation "
         "connection connect connections connect connected connect connecting connect connective connect "
         "was wa this thi say sai yes ye yyy yyi ies i sses ss ing ing eed eed as as is is")


def pairs(text):
    w = text.encode().split()
    return list(zip(w[0::2], w[1::2]))


@pytest.mark.parametrize("step", sorted(PAPER))
def test_reference_against_the_paper(step):
    f = getattr(stem_ref, step)
    for word, want in pairs(PAPER[step]):
        assert f(word) == want, (step, word, f(word))


def test_whole_words():
    for word, want in pairs(WHOLE):
        assert stem_ref.stem(word) == want, (word, stem_ref.stem(word))
        assert tfidf_abi.stem_porter(word) == want, (word, tfidf_abi.stem_porter(word))


def test_host_stemmer_against_reference():
    words = stem_ref.words()
    assert len(words) >= 50_000 and max(len(w) for w in words) <= 64
    changed = 0
    for w in words:
        s = tfidf_abi.stem_porter(w)
        assert s == stem_ref.stem(w), (w, s, stem_ref.stem(w))
        assert 1 <= len(s) <= len(w)
        changed += s != w
    assert changed > len(words) // 2


def test_ineligible_words_and_errors():
    for w in (b"", b"a", b"ed", b"Running", b"runn1ng", b"caf\xc3\xa9s", b"b\x00ing", b"a" * 62 + b"ing"):
        assert tfidf_abi.stem_porter(w) == w == stem_ref.stem(w)
    assert tfidf_abi.stem_porter(b"a" * 61 + b"ing") == b"a" * 61
    assert tfidf_abi.lib().tfidf_stem_porter(None, 3) == tfidf_abi.E_INVAL
    assert tfidf_abi.lib().tfidf_stem_porter(None, 0) == 0


def test_check():
    a, keep = tfidf_abi.analyzer(stem=True)
    assert a.stemmer == tfidf_abi.STEM_PORTER == 1 and tfidf_abi.analyzer_check(a) == 0
    a.stemmer = 2
    assert tfidf_abi.analyzer_check(a) == tfidf_abi.E_INVAL
    a.stemmer = tfidf_abi.STEM_NONE
    assert tfidf_abi.analyzer_check(a) == 0


def both(data, off, **kw):
    """the host function, out of place and in place, against the reference; returns the reference"""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    off = np.asarray(off, dtype=np.uint64)
    ref = stem_ref.analyze(data, off, **kw)
    got = tfidf_abi.analyze_host(data, off, stem=True, **kw)
    assert np.array_equal(got, ref), (bytes(got), bytes(ref))
    assert np.array_equal(tfidf_abi.analyze_host(data, off, stem=True, in_place=True, **kw), ref)
    return bytes(ref)


def test_token_lengths():
    for tail in (b"ing", b"ations"):
        for n in (2, 3, 64, 65):
            tok = (b"ba" * 40)[:max(n - len(tail), 0)] + tail[-min(n, len(tail)):]
            assert len(tok) == n
            buf = b"x " + tok + b" y"
            ref = both(buf, [0, len(buf)])
            if n in (2, 65):
                assert ref == buf
            if n == 64:
                assert ref != buf and ref[2 + 64 - 3:2 + 64] == b"   "


@pytest.mark.parametrize("lower", [False, True])
def test_ineligible_tokens(lower):
    buf = b"runn1ng caf\xc3\xa9s b\x00ing Running running"
    ref = both(buf, [0, len(buf)], lower=lower)
    assert ref == (b"runn1ng caf\xc3\xa9s b\x00ing " + (b"run     " if lower else b"Running ") + b"run    ")


def test_stop_list_sees_the_unstemmed_token():
    buf = b"running run"
    assert both(buf, [0, 11], stop=[b"running"]) == b"        run"
    assert both(buf, [0, 11], stop=[b"run"]) == b"run        "
    assert both(buf, [0, 11], min_len=4) == b"run        "       # min_len against the unstemmed length
    assert both(b"was running", [0, 11], min_len=3) == b"wa  run    "


def test_document_boundary_and_windows():
    assert both(b"running", [0, 4, 7]) == b"running"              # runn | ing
    assert both(b"running", [0, 7]) == b"run    "
    docs = [b"connected connections ", b"agre", b"ed hopping", b"", b" relational sky"]
    data, off = windowed(docs, 37, 21)
    ref = both(data, off, lower=True, punct=True, min_len=2, stop=[b"sky"])
    lo, hi = int(off[0]), int(off[-1])
    assert ref[:lo] == bytes(data[:lo]) and ref[hi:] == bytes(data[hi:])
    assert ref[lo:hi] == b"connect   connect     agr ed hop     relat         "
    data, off = docs_to_arrays([b"ponies", b"", b"caresses"])
    assert both(data, off) == b"poni  caress  "
    assert both(b"running", [3]) == b"running"                     # no documents


def test_without_the_keyword_nothing_changes():
    buf = np.frombuffer(b"running connections", dtype=np.uint8)
    assert bytes(tfidf_abi.analyze_host(buf, [0, len(buf)])) == bytes(buf)
    assert bytes(stem_ref.analyze(buf, [0, len(buf)], stem=False)) == bytes(buf)
    assert bytes(tfidf_abi.analyze_host(buf, [0, 19], True, True, 0, (), False)) == bytes(buf)   # the positional form

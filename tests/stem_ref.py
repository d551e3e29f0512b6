"""The Porter stemmer of the analyzer (include/tfidf.h, section "analyzer", step 3) in plain
Python, one function per step of the 1980 paper, and analyze(): analyze_ref.analyze followed by
the stemming of the surviving tokens.  The only reference of the stemmer tests."""
import numpy as np

import analyze_ref

MAX_WORD = 64

STEP2 = [(b"ational", b"ate"), (b"tional", b"tion"), (b"enci", b"ence"), (b"anci", b"ance"), (b"izer", b"ize"),
         (b"abli", b"able"), (b"alli", b"al"), (b"entli", b"ent"), (b"eli", b"e"), (b"ousli", b"ous"),
         (b"ization", b"ize"), (b"ation", b"ate"), (b"ator", b"ate"), (b"alism", b"al"), (b"iveness", b"ive"),
         (b"fulness", b"ful"), (b"ousness", b"ous"), (b"aliti", b"al"), (b"iviti", b"ive"), (b"biliti", b"ble")]
STEP3 = [(b"icate", b"ic"), (b"ative", b""), (b"alize", b"al"), (b"iciti", b"ic"), (b"ical", b"ic"), (b"ful", b""),
         (b"ness", b"")]
STEP4 = [b"al", b"ance", b"ence", b"er", b"ic", b"able", b"ible", b"ant", b"ement", b"ment", b"ent", b"ion", b"ou",
         b"ism", b"ate", b"iti", b"ous", b"ive", b"ize"]
SUFFIXES = sorted(set([b"sses", b"ies", b"ss", b"s", b"eed", b"ed", b"ing", b"at", b"bl", b"iz", b"y"] +
                      [s for s, _ in STEP2] + [s for s, _ in STEP3] + STEP4))


def is_consonant(w: bytes, i: int) -> bool:
    c = w[i:i + 1]
    if c in (b"a", b"e", b"i", b"o", b"u"):
        return False
    if c == b"y":
        return i == 0 or not is_consonant(w, i - 1)
    return True


def measure(stem: bytes) -> int:
    """m of [C](VC)^m[V]: the number of places where a consonant follows a vowel"""
    return sum(1 for i in range(1, len(stem)) if is_consonant(stem, i) and not is_consonant(stem, i - 1))


def has_vowel(stem: bytes) -> bool:
    return any(not is_consonant(stem, i) for i in range(len(stem)))


def double_consonant(stem: bytes) -> bool:
    return len(stem) >= 2 and stem[-1] == stem[-2] and is_consonant(stem, len(stem) - 1)


def cvc(stem: bytes) -> bool:
    n = len(stem)
    return (n >= 3 and is_consonant(stem, n - 3) and not is_consonant(stem, n - 2) and is_consonant(stem, n - 1)
            and stem[-1:] not in (b"w", b"x", b"y"))


def longest(w: bytes, suffixes):
    """the longest suffix of the list that w ends in, or None"""
    best = None
    for s in suffixes:
        if w.endswith(s) and (best is None or len(s) > len(best)):
            best = s
    return best


def step1a(w: bytes) -> bytes:
    s = longest(w, [b"sses", b"ies", b"ss", b"s"])
    if s == b"sses" or s == b"ies":
        return w[:-2]
    if s == b"s":
        return w[:-1]
    return w


def step1b(w: bytes) -> bytes:
    s = longest(w, [b"eed", b"ed", b"ing"])
    if s is None:
        return w
    stem = w[:-len(s)]
    if s == b"eed":
        return stem + b"ee" if measure(stem) > 0 else w
    if not has_vowel(stem):
        return w
    if stem.endswith((b"at", b"bl", b"iz")):
        return stem + b"e"
    if double_consonant(stem) and stem[-1:] not in (b"l", b"s", b"z"):
        return stem[:-1]
    if measure(stem) == 1 and cvc(stem):
        return stem + b"e"
    return stem


def step1c(w: bytes) -> bytes:
    if w.endswith(b"y") and has_vowel(w[:-1]):
        return w[:-1] + b"i"
    return w


def _replace(w: bytes, rules, min_m: int) -> bytes:
    s = longest(w, [a for a, _ in rules])
    if s is None:
        return w
    stem = w[:-len(s)]
    return stem + dict(rules)[s] if measure(stem) > min_m else w


def step2(w: bytes) -> bytes:
    return _replace(w, STEP2, 0)


def step3(w: bytes) -> bytes:
    return _replace(w, STEP3, 0)


def step4(w: bytes) -> bytes:
    s = longest(w, STEP4)
    if s is None:
        return w
    stem = w[:-len(s)]
    if measure(stem) <= 1:
        return w
    if s == b"ion" and stem[-1:] not in (b"s", b"t"):
        return w
    return stem


def step5a(w: bytes) -> bytes:
    if not w.endswith(b"e"):
        return w
    stem = w[:-1]
    m = measure(stem)
    if m > 1 or (m == 1 and not cvc(stem)):
        return stem
    return w


def step5b(w: bytes) -> bytes:
    if measure(w) > 1 and double_consonant(w) and w.endswith(b"l"):
        return w[:-1]
    return w


STEPS = (step1a, step1b, step1c, step2, step3, step4, step5a, step5b)


def eligible(w: bytes) -> bool:
    return 3 <= len(w) <= MAX_WORD and all(0x61 <= c <= 0x7A for c in w)


def stem(word: bytes) -> bytes:
    w = bytes(word)
    if not eligible(w):
        return w
    for f in STEPS:
        w = f(w)
    return w


_stem = stem   # analyze() has a keyword of the same name


def analyze(data, off, lower=False, punct=False, min_len=0, stop=(), stem=True, stats=None) -> np.ndarray:
    """analyze_ref.analyze, then the stem of every surviving token over its head and 0x20 over
    its tail.  stats (a dict) receives `eligible`, `changed` and `tokens`."""
    out = analyze_ref.analyze(data, off, lower, punct, min_len, stop)
    n_el = n_ch = n_tok = 0
    if stem:
        buf = bytearray(out.tobytes())
        off = [int(x) for x in off]
        cache = {}
        for b, e in zip(off[:-1], off[1:]):
            i = b
            while i < e:
                if buf[i] in analyze_ref.SEPARATORS:
                    i += 1
                    continue
                j = i
                while j < e and buf[j] not in analyze_ref.SEPARATORS:
                    j += 1
                tok = bytes(buf[i:j])
                n_tok += 1
                if eligible(tok):
                    n_el += 1
                    s = cache.get(tok)
                    if s is None:
                        s = cache[tok] = _stem(tok)
                    assert 1 <= len(s) <= len(tok)
                    if s != tok:
                        n_ch += 1
                        buf[i:j] = s + b" " * (len(tok) - len(s))
                i = j
        out = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    if stats is not None:
        stats.update(eligible=n_el, changed=n_ch, tokens=n_tok)
    return out



# ---- the words of the tests ----

STEMS = [b"a", b"b", b"tr", b"y", b"ay", b"by", b"oat", b"be", b"ee", b"hop", b"fil", b"fail", b"fizz", b"hiss", b"fall",
         b"contr", b"abl", b"siz", b"yy", b"eye", b"troubl", b"conflat", b"agr", b"sens", b"ration", b"gener"]
WORD_SUFFIXES = SUFFIXES + [b"e", b"ll", b"es", b"ying", b"pping", b"ated", b"bled", b"ized"]


def words():
    """every stem followed by one or two suffixes, at most 64 bytes, in a fixed order"""
    out = []
    for s in STEMS:
        for a in WORD_SUFFIXES:
            out.append(s + a)
            out.extend(s + a + b for b in WORD_SUFFIXES)
    return [w for w in out if len(w) <= MAX_WORD]

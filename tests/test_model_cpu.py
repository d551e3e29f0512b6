"""Host-only pieces of the portable model (include/tfidf.h, section "model"): tfidf_model_check's
rules one by one, and the file format of tfidf_model_save / tfidf_model_load against a file this
test assembles itself.  No GPU call."""
import struct

import numpy as np
import pytest

import oracle_py
import tfidf_abi
from conftest import golden_cases
from helpers import load_golden

SEPARATORS = [0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D]


def model_of(terms, df, N):
    return {"N": N, "terms": list(terms), "df": np.asarray(df, dtype=np.uint32)}


def golden_model(case):
    """the term table of a golden corpus from the oracle, in strcmp("word\\t") order"""
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    df = {}
    for t, d in zip(ora["term"].tolist(), ora["df"].tolist()):
        df[ora["terms"][t]] = d
    terms = sorted(df, key=lambda w: w + b"\t")
    return model_of(terms, [df[w] for w in terms], len(g["off"]) - 1)


def raw(model):
    """the model with explicit term_off / term_bytes arrays, to break them"""
    terms = model["terms"]
    off = np.zeros(len(terms) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(t) for t in terms], dtype=np.uint64)
    return {"N": model["N"], "df": model["df"].copy(), "term_off": off,
            "term_bytes": np.frombuffer(b"".join(terms), dtype=np.uint8).copy()}


EDGE = model_of(sorted([b"", b"a" * 15, b"b" * 16, b"c" * 17, b"\x80\xff\xfe", b"ab", b"ab\x01", b"zz"],
                       key=lambda w: w + b"\t"), [1, 2, 3, 4, 5, 6, 7, 7], 7)


# ---- tfidf_model_check ----

@pytest.mark.parametrize("case", golden_cases())
def test_check_accepts_every_golden(case):
    m = golden_model(case)
    assert tfidf_abi.model_check(m) == 0
    assert tfidf_abi.model_check(raw(m)) == 0


def test_check_accepts_edge_terms():
    assert EDGE["terms"][0] == b"" and EDGE["terms"].index(b"ab\x01") + 1 == EDGE["terms"].index(b"ab")
    assert tfidf_abi.model_check(EDGE) == 0
    assert tfidf_abi.model_check(model_of([], [], 0)) == 0          # no term: valid for any N
    assert tfidf_abi.model_check(model_of([], [], 1 << 40)) == 0
    assert tfidf_abi.model_check(model_of([b""], [1], 1)) == 0


def broken(name):
    good = model_of([b"ab\x01", b"ab", b"b", b"c"], [1, 2, 3, 3], 3)
    assert tfidf_abi.model_check(good) == 0
    t, df = list(good["terms"]), good["df"].copy()
    if name == "swapped":
        t[2], t[3] = t[3], t[2]
    elif name == "duplicate":
        t[3] = t[2]
    elif name == "tab_rule":           # "ab\x01\t" < "ab\t": ab placed first is out of order
        t[0], t[1] = t[1], t[0]
    elif name == "nul":
        t[2] = b"b\0"
    elif name.startswith("sep_"):
        t[3] = b"c" + bytes([int(name[4:], 16)]) + b"d"
    elif name == "df_zero":
        df[1] = 0
    elif name == "df_over_n":
        df[1] = 4
    return model_of(t, df, 3)


@pytest.mark.parametrize("name", ["swapped", "duplicate", "tab_rule", "nul", "df_zero", "df_over_n"] +
                         ["sep_%02x" % s for s in SEPARATORS])
def test_check_rejects(name):
    assert tfidf_abi.model_check(broken(name)) == tfidf_abi.E_INVAL


def test_check_rejects_decreasing_offsets_and_short_size():
    r = raw(model_of([b"a", b"bc", b"d"], [1, 1, 1], 1))
    assert tfidf_abi.model_check(r) == 0
    assert tfidf_abi.model_check(r, size=tfidf_abi.C.sizeof(tfidf_abi.Model) - 1) == tfidf_abi.E_INVAL
    assert tfidf_abi.model_check(r, size=tfidf_abi.C.sizeof(tfidf_abi.Model) + 8) == 0   # a longer, newer struct
    r["term_off"] = np.array([0, 3, 1, 4], dtype=np.uint64)
    assert tfidf_abi.model_check(r) == tfidf_abi.E_INVAL


# ---- the file ----

def fnv1a(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def file_of(model, version=1, magic=b"TFIDFMDL") -> bytes:
    """the file of include/tfidf.h's table, assembled here"""
    terms, V = model["terms"], len(model["terms"])
    off = [0]
    for t in terms:
        off.append(off[-1] + len(t))
    payload = struct.pack("<%dQ" % (V + 1), *off) + struct.pack("<%dI" % V, *model["df"].tolist()) + b"".join(terms)
    return magic + struct.pack("<IIQQQ", version, V, model["N"], off[-1], fnv1a(payload)) + payload


def same_model(a, b):
    assert a["N"] == b["N"] and a["terms"] == list(b["terms"])
    assert np.array_equal(a["df"], b["df"])


@pytest.mark.parametrize("model", [EDGE, model_of([], [], 5), golden_model("g3_bytes"), golden_model("g5_w3")],
                         ids=["edge", "empty", "g3_bytes", "g5_w3"])
def test_save_load_round_trip_and_bytes(tmp_path, model):
    p, q = str(tmp_path / "m.bin"), str(tmp_path / "n.bin")
    tfidf_abi.model_save(model, p)
    got = tfidf_abi.model_load(p)
    same_model(got, model)
    assert got["term_off"][0] == 0 and bytes(got["term_bytes"]) == b"".join(model["terms"])
    data = open(p, "rb").read()
    assert data == file_of(model)
    tfidf_abi.model_save(got, q)                      # twice, and from the loaded arrays: the same bytes
    tfidf_abi.model_save(model, p)
    assert open(q, "rb").read() == data == open(p, "rb").read()


def test_save_rebases_offsets_and_checks(tmp_path):
    r = raw(model_of([b"a", b"bc"], [1, 2], 2))
    r["term_bytes"] = np.frombuffer(b"xyz" + bytes(r["term_bytes"]), dtype=np.uint8).copy()
    r["term_off"] = r["term_off"] + np.uint64(3)
    tfidf_abi.model_save(r, str(tmp_path / "m.bin"))
    assert open(tmp_path / "m.bin", "rb").read() == file_of(model_of([b"a", b"bc"], [1, 2], 2))
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_save(broken("swapped"), str(tmp_path / "bad.bin"))
    assert ex.value.rc == tfidf_abi.E_INVAL
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_save(EDGE, str(tmp_path / "no" / "such" / "dir.bin"))
    assert ex.value.rc == tfidf_abi.E_OUTPUT


def load_rc(tmp_path, data) -> int:
    p = tmp_path / "x.bin"
    p.write_bytes(data)
    try:
        tfidf_abi.model_load(str(p))
    except tfidf_abi.TfidfError as e:
        return e.rc
    return 0


def test_load_rejects(tmp_path):
    good = file_of(EDGE)
    assert load_rc(tmp_path, good) == 0
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_load(str(tmp_path / "missing.bin"))
    assert ex.value.rc == tfidf_abi.E_MODEL
    flipped = bytearray(good)
    flipped[-3] ^= 0x04
    unordered = file_of(model_of([b"b", b"a"], [1, 1], 1))     # its checksum is right
    cases = {
        "cut": good[:-1], "extra": good + b"\0", "flipped": bytes(flipped), "magic": file_of(EDGE, magic=b"TFIDFMDX"),
        "version": file_of(EDGE, version=2), "unordered": unordered, "header only": good[:40], "empty": b"",
    }
    for name, data in cases.items():
        assert load_rc(tmp_path, data) == tfidf_abi.E_MODEL, name
    assert tfidf_abi.lib().tfidf_strerror(tfidf_abi.E_MODEL) not in (b"unknown error", None)

"""CPU-side checks of tfidf_transform's product boundary (no GPU compute calls): the symbols
and the binding's export list, argument errors that need no device, tfidf_rows_free on empty
structs, and the ctypes structs against include/tfidf.h."""
import ctypes as C
import os
import re

import tfidf_abi
from conftest import REPO

NEW = ["tfidf_transform", "tfidf_rows_free", "tfidf_group_transform", "tfidf_last_transform_info"]


def test_exports():
    lib = tfidf_abi.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in tfidf_abi.EXPORTS, name
    assert lib.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2    # the change is additive
    for name in ("Rows", "TransformInfo"):
        assert hasattr(tfidf_abi, name)
    for cls, names in ((tfidf_abi.Engine, ("transform", "transform_corpus", "transform_info")),
                       (tfidf_abi.Group, ("transform",))):
        for n in names:
            assert callable(getattr(cls, n)), n


def test_null_arguments_are_invalid():
    lib = tfidf_abi.lib()
    c, r = tfidf_abi.Corpus(), tfidf_abi.Rows()
    fake = C.c_void_p(1)   # never dereferenced: the NULL checks come first
    assert lib.tfidf_transform(None, C.byref(c), C.byref(r)) == tfidf_abi.E_INVAL
    assert lib.tfidf_transform(fake, None, C.byref(r)) == tfidf_abi.E_INVAL
    assert lib.tfidf_transform(fake, C.byref(c), None) == tfidf_abi.E_INVAL
    assert lib.tfidf_group_transform(None, C.byref(c), C.byref(r)) == tfidf_abi.E_INVAL
    assert lib.tfidf_group_transform(fake, None, C.byref(r)) == tfidf_abi.E_INVAL
    assert lib.tfidf_group_transform(fake, C.byref(c), None) == tfidf_abi.E_INVAL
    ti = tfidf_abi.TransformInfo()
    ti.size = C.sizeof(ti)
    assert lib.tfidf_last_transform_info(None, C.byref(ti)) == tfidf_abi.E_INVAL
    assert lib.tfidf_last_transform_info(fake, None) == tfidf_abi.E_INVAL


def test_rows_free_of_nothing():
    lib = tfidf_abi.lib()
    lib.tfidf_rows_free(None)
    r = tfidf_abi.Rows()
    lib.tfidf_rows_free(C.byref(r))
    lib.tfidf_rows_free(C.byref(r))
    assert bytes(r) == bytes(C.sizeof(r))


_SIZES = {"uint32_t": 4, "uint64_t": 8, "double": 8}


def header_struct(name: str):
    """(field, size) of a typedef'd struct of include/tfidf.h, in order"""
    with open(os.path.join(REPO, "include", "tfidf.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)(\s*\*)?\s*(.+)$", decl)
        ty, ptr, names = m.group(1), m.group(2), m.group(3)
        for n in names.split(","):
            out.append((n.strip(), 8 if ptr else _SIZES[ty]))
    return out


def test_structs_mirror_the_header():
    for cname, cls in (("tfidf_rows", tfidf_abi.Rows), ("tfidf_transform_info", tfidf_abi.TransformInfo)):
        want = header_struct(cname)
        assert [n for n, _ in want] == [n for n, _ in cls._fields_], cname
        at = 0
        for n, size in want:    # natural alignment, as the C compiler lays the struct out
            at = (at + size - 1) // size * size
            f = getattr(cls, n)
            assert (f.offset, f.size) == (at, size), (cname, n)
            at += size
        assert C.sizeof(cls) == (at + 7) // 8 * 8, cname
    assert C.sizeof(tfidf_abi.Rows) == 96 and C.sizeof(tfidf_abi.TransformInfo) == 88

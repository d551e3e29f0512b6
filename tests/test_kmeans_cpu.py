"""CPU-side checks of tfidf_kmeans's product boundary (no GPU compute calls): the reference
implementation (kmeans_ref.py) on a case worked by hand, the exported symbols and the binding,
argument errors that need no device, and the ctypes structs against a C compiler's layout of
include/tfidf.h."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfidf_abi
from conftest import REPO
from kmeans_ref import KRef, NO_CLUSTER, cluster_lines

NEW = ["tfidf_kmeans", "tfidf_clusters_free", "tfidf_last_kmeans_info"]


def hand_ora():
    """Four documents over the terms a < b < c whose scores are chosen, not computed:
         doc1 = (a 3, b 4)   doc2 = (a 1)   doc3 = (b 2, c 2)   doc4 = (c 5)
    The oracle numbers terms in any order (here c, a, b): the reference ranks them by name."""
    terms = [b"c", b"a", b"b"]
    rows = [(1, b"a", 3.0), (1, b"b", 4.0), (2, b"a", 1.0), (3, b"b", 2.0), (3, b"c", 2.0), (4, b"c", 5.0)]
    return dict(terms=terms, doc=np.array([r[0] for r in rows], dtype=np.uint32),
                term=np.array([terms.index(r[1]) for r in rows], dtype=np.uint32),
                score=np.array([r[2] for r in rows], dtype=np.float64))


def test_reference_on_a_hand_worked_case():
    """K = 2, seeds doc1 and doc4.  Unit vectors: u1 = (.6, .8, 0), u2 = (1, 0, 0),
    u3 = (r, r) on (b, c) with r = 2 / sqrt(8), u4 = (0, 0, 1).
    Pass 1 against C0 = u1, C1 = u4: sims doc1 (1, 0) -> fl(.36) + fl(.64), doc2 (.6, 0),
    doc3 (fl(r * .8), r): r = .7071.. > .5657.. so doc3 goes to cluster 1, doc4 (0, 1).
    Labels 0 0 1 1.  Update: S0 = (1.6, .8, 0), S1 = (0, r, r + 1).  Pass 2 keeps the labels
    (doc3: r * r / n1 vs r * .8 / n0 + ..), so the loop stops converged after 2 passes and the
    sims are those against the updated centroids."""
    ref = KRef(hand_ora(), [1, 2, 3, 4])
    assert ref.words == [b"a", b"b", b"c"] and ref.order == [1, 2, 3, 4]
    r = 2.0 / math.sqrt(8.0)
    assert ref.u[0].tolist() == [3.0 / 5.0, 4.0 / 5.0] and ref.u[2].tolist() == [r, r] and ref.u[3].tolist() == [1.0]
    one = ref.run(2, max_iter=1, nterms=3, seeds=[1, 4])
    assert (one["iterations"], one["converged"]) == (1, 0)
    assert one["label"] == [0, 0, 1, 1] and one["size"] == [2, 2]
    assert one["sim"] == [0.6 * 0.6 + 0.8 * 0.8, 0.6, r, 1.0]
    assert one["top"][0] == [(1, 0.8, b"b"), (0, 0.6, b"a")] and one["top"][1] == [(2, 1.0, b"c")]
    res = ref.run(2, max_iter=20, nterms=3, seeds=[1, 4])
    assert (res["iterations"], res["converged"]) == (2, 1) and res["label"] == [0, 0, 1, 1]
    n0 = math.sqrt(1.6 * 1.6 + 0.8 * 0.8)
    s1b, s1c = 0.0 + r, (0.0 + r) + 1.0
    n1 = math.sqrt(s1b * s1b + s1c * s1c)
    c0, c1 = (1.6 / n0, 0.8 / n0), (s1b / n1, s1c / n1)
    assert res["cents"][0] == {0: c0[0], 1: c0[1]} and res["cents"][1] == {1: c1[0], 2: c1[1]}
    assert res["sim"] == [0.6 * c0[0] + 0.8 * c0[1], 1.0 * c0[0], r * c1[0] + r * c1[1], 1.0 * c1[1]]
    assert res["top"][0] == [(0, c0[0], b"a"), (1, c0[1], b"b")] and res["top"][1] == [(2, c1[1], b"c"), (1, c1[0], b"b")]
    assert cluster_lines(res).startswith(b"c0\t2\ta:%.16f b:%.16f\nc1\t2\tc:" % c0)
    assert cluster_lines(res).endswith(b"doc4\tc1\t%.16f\n" % c1[1])
    # default seeds: the clusterable documents at floor(c * M / K)
    assert ref.default_seeds(2) == [1, 3] and ref.default_seeds(4) == [1, 2, 3, 4] and ref.default_seeds(3) == [1, 2, 3]
    # the seed rules
    for bad in ([1, 1], [1, 9], [1], [1, 2, 3]):
        assert ref.run(2, seeds=bad) is None
    assert ref.run(5) is None and ref.run(0) is None


def test_reference_unclustered_and_ties():
    """doc2 has no pairs and doc3 only a zero score: unclustered.  doc1 and doc4 are equal, so
    every sim ties and everything goes to cluster 0; cluster 1 stays empty and keeps its seed."""
    terms = [b"x", b"y"]
    rows = [(1, 0, 2.0), (3, 1, 0.0), (4, 0, 2.0), (5, 0, 1.0), (5, 1, 0.0)]
    ora = dict(terms=terms, doc=np.array([r[0] for r in rows], dtype=np.uint32),
               term=np.array([r[1] for r in rows], dtype=np.uint32), score=np.array([r[2] for r in rows]))
    ref = KRef(ora, [1, 2, 3, 4, 5])
    assert ref.clusterable == [0, 3, 4]
    res = ref.run(2, seeds=[1, 4])
    assert res["label"] == [0, NO_CLUSTER, NO_CLUSTER, 0, 0] and res["size"] == [3, 0]
    assert res["sim"][1] == 0.0 and res["top"][1] == [(0, 1.0, b"x")] and res["converged"] == 1
    assert ref.run(2, seeds=[1, 3]) is None and ref.run(4) is None
    assert b"doc2\t-\t0.0000000000000000\n" in cluster_lines(res)


def test_exports():
    lib = tfidf_abi.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in tfidf_abi.EXPORTS, name
    assert lib.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2    # the change is additive
    for name in ("KmeansParams", "Clusters", "KmeansInfo"):
        assert hasattr(tfidf_abi, name)
    for n in ("kmeans", "kmeans_info"):
        assert callable(getattr(tfidf_abi.Engine, n)), n
    assert tfidf_abi.NO_CLUSTER == NO_CLUSTER and tfidf_abi.KMEANS_MAX_K == 256 and tfidf_abi.KMEANS_MAX_TERMS == 64


def test_null_and_short_arguments_are_invalid():
    lib = tfidf_abi.lib()
    p, c = tfidf_abi.KmeansParams(), tfidf_abi.Clusters()
    p.size, p.k = C.sizeof(p), 2
    fake = C.c_void_p(1)   # never dereferenced: these checks come first
    assert lib.tfidf_kmeans(None, C.byref(p), C.byref(c)) == tfidf_abi.E_INVAL
    assert lib.tfidf_kmeans(fake, None, C.byref(c)) == tfidf_abi.E_INVAL
    assert lib.tfidf_kmeans(fake, C.byref(p), None) == tfidf_abi.E_INVAL
    p.size = C.sizeof(p) - 1
    assert lib.tfidf_kmeans(fake, C.byref(p), C.byref(c)) == tfidf_abi.E_INVAL
    p.size = C.sizeof(p)
    for k, t in ((0, 1), (257, 1), (2, 65)):
        p.k, p.nterms = k, t
        assert lib.tfidf_kmeans(fake, C.byref(p), C.byref(c)) == tfidf_abi.E_INVAL
    seeds = (C.c_uint32 * 3)(1, 2, 3)
    p.k, p.nterms, p.seeds, p.nseeds = 2, 1, C.cast(seeds, C.POINTER(C.c_uint32)), 3
    assert lib.tfidf_kmeans(fake, C.byref(p), C.byref(c)) == tfidf_abi.E_INVAL
    ki = tfidf_abi.KmeansInfo()
    ki.size = C.sizeof(ki)
    assert lib.tfidf_last_kmeans_info(None, C.byref(ki)) == tfidf_abi.E_INVAL
    assert lib.tfidf_last_kmeans_info(fake, None) == tfidf_abi.E_INVAL
    lib.tfidf_clusters_free(None)
    lib.tfidf_clusters_free(C.byref(c))
    assert bytes(c) == bytes(C.sizeof(c))


SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "tfidf.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(tfidf_kmeans_params), sizeof(tfidf_clusters), sizeof(tfidf_kmeans_info),
           offsetof(tfidf_kmeans_params, seeds), offsetof(tfidf_clusters, doc), offsetof(tfidf_clusters, word_bytes),
           offsetof(tfidf_kmeans_info, ms_total));
    printf("%u %u %u\n", TFIDF_KMEANS_MAX_K, TFIDF_KMEANS_MAX_TERMS, TFIDF_NO_CLUSTER);
    return 0;
}
"""


def test_structs_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler: the library's own build needs one")
    (tmp_path / "sizes.c").write_text(SIZES_C)
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "sizes"), str(tmp_path / "sizes.c")],
                   check=True, timeout=120)
    out = subprocess.run([str(tmp_path / "sizes")], capture_output=True, check=True, timeout=60).stdout.split()
    got = [int(x) for x in out]
    a = tfidf_abi
    assert got[:7] == [C.sizeof(a.KmeansParams), C.sizeof(a.Clusters), C.sizeof(a.KmeansInfo), a.KmeansParams.seeds.offset,
                       a.Clusters.doc.offset, a.Clusters.word_bytes.offset, a.KmeansInfo.ms_total.offset]
    assert got[7:] == [a.KMEANS_MAX_K, a.KMEANS_MAX_TERMS, a.NO_CLUSTER]
    assert got[:3] == [32, 104, 88]

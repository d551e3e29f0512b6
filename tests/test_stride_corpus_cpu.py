"""The properties test_gpu_grid_stride.py relies on, established without a GPU from the oracle's
result on the stride corpus (tests/stride_corpus.py), the name-order output positions and the
constants of csrc/kernels.h.  These are conditions on the corpus, not measurements: when a cap or
a cut in kernels.h changes and one of them fails, the generator is what has to follow."""
import numpy as np
import pytest

import dedup_ref
import oracle_py
import stride_corpus as SC
from helpers import docs_to_arrays


@pytest.fixture(scope="module")
def sc():
    c = SC.build()
    data, off = docs_to_arrays(c["docs"])
    ora = oracle_py.run(data, off)
    per_id = np.bincount(ora["doc"], minlength=SC.NDOCS + 1)
    n = [int(per_id[d]) for d in c["order"]]                    # pairs by output position
    ref = dedup_ref.DRef(ora, range(1, SC.NDOCS + 1))
    dups = ref.near_dups(64, 1, 1, 0.0)
    bigcand = [(a, b) for a, b in dups["cand"] if max(n[a], n[b]) > SC.DD_BIG_PAIRS]
    return dict(c=c, ora=ora, n=n, ref=ref, dups=dups, bigcand=bigcand)


def test_the_oracle_counts_what_the_generator_laid_out(sc):
    c, ora, n = sc["c"], sc["ora"], sc["n"]
    assert SC.QS_BIG == SC.RW_BIG == SC.DD_BIG_PAIRS                # one cut: a big document is big for every call
    assert sc["ref"].order == c["order"] and n == c["sizes"]
    assert set(SC.SIZES) <= set(n)
    assert len(n) == SC.NDOCS == 300 and ora["npairs"] <= 85000      # small: the references are plain Python loops
    assert 2000 <= ora["nterms"] <= 8000
    assert {15, 16, 17} <= {len(w) for w in ora["terms"]}
    assert set(ora["count"].tolist()) == {1, 2, 3}


def test_big_documents_are_many_spread_and_apart(sc):
    n, big = sc["n"], sc["c"]["big"]
    assert [p for p, x in enumerate(n) if x > SC.BIG] == big and all(n[p] == SC.BIG + 1 for p in big)
    assert len(big) >= 13 and min(b - a for a, b in zip(big, big[1:])) > 1
    assert all(any(q * SC.NDOCS // 4 <= p < (q + 1) * SC.NDOCS // 4 for p in big) for q in range(4))
    sets = sc["ref"].sets
    for a, b in zip(big, big[1:]):                                  # near-identical: all but ~100 terms shared
        assert SC.BIG + 1 - len(np.intersect1d(sets[a], sets[b])) <= 2 * SC.BLOCK


def test_families_of_identical_small_documents(sc):
    c = sc["c"]
    for fam in c["families"]:
        assert len(fam) >= 12 and len({c["docs"][c["order"][p] - 1] for p in fam}) == 1
        assert 0 < sc["n"][fam[0]] <= SC.BIG
    assert sum(len(f) - 1 for f in c["families"]) >= 22


def test_three_trips_per_loop(sc):
    """TFIDF_GRID_CUS=1: every grid-stride loop of the table makes at least three trips"""
    n, dups = sc["n"], sc["dups"]
    nbig = sum(1 for x in n if x > SC.BIG)
    per_cu = SC.PER_CU
    assert len(n) >= 3 * SC.WAVES * max(per_cu[c] for c in SC.WAVE_KERNELS.values()) + 1
    assert len(n) >= 3 * max(per_cu[c] for c in SC.ROW_KERNELS.values()) + 1
    assert nbig >= 3 * max(per_cu["BIG_WG_PER_CU"], per_cu["DD_BIG_WG_PER_CU"], per_cu["TM_BIG_WG_PER_CU"]) + 1
    assert -(-sc["ora"]["npairs"] // SC.PR_TILE) >= 3 * per_cu["PR_WG_PER_CU"] + 1
    t = SC.trips(1, len(n), nbig, sc["ora"]["npairs"], dups["ncand"], len(sc["bigcand"]))
    print(t)
    assert len(t) == 16 and all(v >= 3 for v in t.values()), t
    # with the device's own count nothing here takes a second trip: what the suite saw before
    assert set(SC.trips(256, len(n), nbig, sc["ora"]["npairs"], dups["ncand"], len(sc["bigcand"])).values()) == {1}


@pytest.mark.parametrize("S", SC.STRIDES)
def test_wave_transitions(sc, S):
    """a wave (or a one-wave workgroup) that steps S positions meets, one right after the other:"""
    n = sc["n"]
    steps = [(n[p], n[p + S]) for p in range(len(n) - S)]
    assert any(a >= 64 and b == 0 for a, b in steps)                          # pairs, then an empty document
    assert any(a > SC.BIG and 0 < b <= SC.BIG for a, b in steps)              # big (handed on), then small
    assert any(0 < n[p] <= SC.BIG < n[p + S] and 0 < n[p + 2 * S] <= SC.BIG for p in range(len(n) - 2 * S))
    assert any(SC.BIG >= a > SC.RW_KEEP and 0 < b <= SC.RW_KEEP for a, b in steps)   # reloaded w, then w in registers


def test_candidates(sc):
    """near_dups(64, 1, 1, 0.0): more candidates than three trips of the verification's waves, enough of
    them with a big document for three trips of its workgroups, and small ones beside them"""
    dups, bigcand = sc["dups"], sc["bigcand"]
    per_cu = SC.PER_CU
    assert dups["ncand"] >= max(97, 3 * SC.WAVES * per_cu["DD_WG_PER_CU"] + 1)
    assert len(bigcand) >= max(13, 3 * per_cu["DD_BIG_WG_PER_CU"] + 1)
    assert dups["ncand"] - len(bigcand) > 32 * 3
    big = set(sc["c"]["big"])
    assert sum(1 for a, b in bigcand if a in big and b in big) >= 12          # big against big
    assert any((a in big) != (b in big) for a, b in bigcand)                  # big against small: unequal lists

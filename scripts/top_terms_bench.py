#!/usr/bin/env python3
"""Per-document top-k keywords over a resident result (tfidf_top_terms): config 2 generated
and run on the GPU, then the k best words of every document at k = 10 and k = 1024.

Reports, after two warm-up calls, the median over --reps calls of the call's device times
(HIP events inside the library: lookup, selection, word scan + gather) and host wall time of
the C call (its D2H copies into the caller's arrays included); the selection pass's nominal
bytes (8 P of scores read, the rows' 32 bytes per entry and 16 per row written) over its time
as a fraction of the measured streaming-read peak (tfidf_hbm_probe); and tfidf_fetch of the
same run, the copy of every pair the call exists to avoid.

    python3 scripts/top_terms_bench.py [--scale S] [--commit ID] [--out profiles/top_terms_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "python"))
import tfidf_abi  # noqa: E402
import tfidf_configs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--k", type=int, nargs="+", default=[10, 1024])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

p = tfidf_configs.plan(args.config, scale=args.scale)
L = tfidf_abi.lib()
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    fetch_ms = []
    for _ in range(3):                             # tfidf_fetch of the same run: every pair to the host
        t0 = time.perf_counter()
        with e.fetched():
            fetch_ms.append((time.perf_counter() - t0) * 1e3)
    probe = e.hbm_probe(1 << 30, 5)

    def call(k):
        """the C call alone: the rows stay in the library's arrays and are released"""
        t = tfidf_abi.DocTerms()
        t1 = time.perf_counter()
        rc = L.tfidf_top_terms(e.h, None, 0, k, C.byref(t))
        wall = (time.perf_counter() - t1) * 1e3
        assert rc == 0, rc
        words = int(t.word_off[int(t.ndocs) * k])
        L.tfidf_doc_terms_free(C.byref(t))
        ti = e.terms_info()
        ti["wall_ms"] = wall
        ti["word_bytes"] = words
        return ti

    per_k = {}
    for k in args.k:
        call(k)
        call(k)                                    # warm-up: code objects, the context's buffers
        a0 = e.alloc_counters()
        rows = [call(k) for _ in range(args.reps)]
        allocs = e.alloc_counters()[0] - a0[0]
        med = {x: statistics.median(r[x] for r in rows) for x in ("ms_lookup", "ms_select", "ms_words", "ms_total", "wall_ms")}
        nominal = 8 * P + N * k * 32 + N * 16
        gbps = nominal / (med["ms_select"] * 1e-3) / 1e9 if med["ms_select"] > 0 else 0.0
        per_k[str(k)] = {
            "ms": {x: round(v, 4) for x, v in med.items()},
            "select_ms_min_max": [round(min(r["ms_select"] for r in rows), 4), round(max(r["ms_select"] for r in rows), 4)],
            "nbatches": rows[-1]["nbatches"], "big_docs": rows[-1]["big_docs"], "out_bytes": rows[-1]["out_bytes"],
            "word_bytes": rows[-1]["word_bytes"], "device_allocs_in_timed_calls": allocs,
            "select_nominal_bytes": nominal, "select_GBps": round(gbps, 1),
            "select_fraction_of_read_peak": round(gbps / probe["read_GBps"], 4) if probe["read_GBps"] > 0 else None,
            "faster_than_fetch": med["wall_ms"] < statistics.median(fetch_ms),
        }
    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "reps": args.reps, "k": per_k, "hbm_read_peak_GBps": round(probe["read_GBps"], 1),
        "fetch_ms": round(statistics.median(fetch_ms), 2), "fetch_ms_all": [round(x, 2) for x in fetch_ms],
        "fetch_bytes": 16 * P,
        "note": "device times are HIP events inside tfidf_top_terms; wall_ms is the C call, with its host "
                "allocations and the D2H of the rows into pageable memory; select bytes are nominal",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

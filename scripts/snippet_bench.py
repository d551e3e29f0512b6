#!/usr/bin/env python3
"""Snippets over a resident corpus (tfidf_snippet): config 2 generated on the host and run on the
GPU, then batches of 64 and 4096 queries of 4 Zipf-drawn vocabulary words at k = 10; the jobs are
the hits of tfidf_query, W = 32.

Reports per batch, after warm-up calls, the median and min-max over --reps calls of the device
times (HIP events inside the library: lookup, count, write, select, emit) and of the host wall
time; the tfidf_query call that produced the hits, measured the same way in the same session; the
same jobs through tfidf_result_snippet (plain C, one host thread), once; and the count pass's
document bytes per second next to the measured streaming-read peak (tfidf_hbm_probe).

    python3 scripts/snippet_bench.py [--scale S] [--commit ID] [--out profiles/snippets_c2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "python"))
import numpy as np  # noqa: E402
import tfidf_abi  # noqa: E402
import tfidf_configs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--batches", default="64,4096")
ap.add_argument("--words", type=int, default=4)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


p = tfidf_configs.plan(args.config, scale=args.scale)
data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
with tfidf_abi.Engine(0) as e:
    e.run_host(data, off, p["doc_ids"], p["ndocs_total"])
    info = e.info()
    res = e.fetch()
    terms = res["terms"]
    by_df = np.argsort(-res["term_df"].astype(np.int64), kind="stable")
    cdf = tfidf_configs.zipf_cdf(len(terms), 1.07)
    probe = e.hbm_probe(1 << 30, 5)
    out = {"commit": args.commit, "config": args.config, "scale": args.scale, "docs": info["ndocs"], "terms": len(terms),
           "corpus_bytes": int(len(data)), "words_per_query": args.words, "k": args.k, "window": args.window,
           "reps": args.reps, "hbm_read_peak_GBps": round(probe["read_GBps"], 1), "batches": {}}
    for nq in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(1)
        queries = [b" ".join(terms[int(t)] for t in by_df[np.searchsorted(cdf, rng.random(args.words))])
                   for _ in range(nq)]
        hits = e.query(queries, args.k)
        jobs = tfidf_abi.hits_to_jobs(hits)
        params = tfidf_abi.snippet_params(window=args.window)
        qrows, srows = [], []
        for i in range(2 + args.reps):                 # two warm-up calls of each: code objects, the context's buffers
            t0 = time.perf_counter()
            e.query(queries, args.k)
            qi = e.query_info()
            qi["wall_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            got = e.snippets(queries, jobs, params=params)
            si = e.snippet_info()
            si["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if i >= 2:
                qrows.append(qi)
                srows.append(si)
        t0 = time.perf_counter()
        twin = tfidf_abi.result_snippets(res, data, off, queries, jobs, doc_ids=p["doc_ids"], params=params)
        twin_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(got[k], twin[k]) for k in ("ntokens", "nmatch", "win_tok", "win_byte", "cover", "hits"))
        last = srows[-1]
        m = {"jobs": len(jobs), "tiles": last["ntiles"], "bytes_scanned": last["nbytes"], "tokens": last["ntokens"],
             "matches": last["nmatches"], "nbatches": last["nbatches"], "nsubbatches": last["nsubbatches"],
             "snippet_ms": {k: stat([r[k] for r in srows]) for k in ("ms_lookup", "ms_count", "ms_write", "ms_select", "ms_emit",
                                                                      "ms_total", "wall_ms")},
             "query_ms": {k: stat([r[k] for r in qrows]) for k in ("ms_lookup", "ms_score", "ms_topk", "ms_total", "wall_ms")},
             "twin_one_thread_ms": round(twin_ms, 2), "twin_equal": bool(same)}
        cnt = m["snippet_ms"]["ms_count"]["median"]
        m["count_GBps"] = round(last["nbytes"] / (cnt * 1e-3) / 1e9, 2) if cnt > 0 else None
        m["twin_over_device_wall"] = round(twin_ms / m["snippet_ms"]["wall_ms"]["median"], 2)
        m["snippet_over_query_wall"] = round(m["snippet_ms"]["wall_ms"]["median"] / m["query_ms"]["wall_ms"]["median"], 3)
        out["batches"][str(nq)] = m
    out["note"] = ("device times are HIP events inside the calls; wall_ms is the Python call and includes host tokenising, "
                   "uploads, the read-backs between the passes and the conversion of the result arrays")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

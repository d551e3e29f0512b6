#!/usr/bin/env python3
"""BM25 ranking over a resident result (tfidf_query_bm25) next to tfidf_query: config 2
generated and run on the GPU, then the batch of scripts/query_bench.py (64 queries of 4
Zipf-drawn vocabulary words, k = 10) through both entry points on the same run.

The two are called alternately; after 2 warm-up calls each, the median over --reps calls of
the device times (HIP events inside the library: lookup, scoring, top-k) and the host wall
time is reported for both, with the ratio of the scoring passes.  Two figures say where a
ratio above 1 comes from: the same comparison for a batch of uniformly drawn (rare) words,
whose pass is the scan of the terms with next to no match (table staging and filter only),
and the extra scoring time per matched pair of the Zipf batch (one K(d)-normalised division
and one count load each).

    python3 scripts/bm25_bench.py [--scale S] [--commit ID] [--out profiles/bm25_c2.json]
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
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--words", type=int, default=4)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

KEYS = ("ms_lookup", "ms_score", "ms_topk", "ms_total", "wall_ms")

p = tfidf_configs.plan(args.config, scale=args.scale)
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    with e.fetched() as r:
        df = r["term_df"].astype(np.int64)
        by_df = np.argsort(-df, kind="stable")
        toff, tb = r["term_off"], r["term_bytes"]
        rng = np.random.default_rng(1)
        cdf = tfidf_configs.zipf_cdf(V, 1.07)     # query_bench.py's batch: Zipf over the words by descending df
        word = lambda t: bytes(tb[int(toff[t]):int(toff[t + 1])])
        zipf_terms = [by_df[np.searchsorted(cdf, rng.random(args.words))].tolist() for _ in range(args.queries)]
        rare_terms = [rng.integers(0, V, args.words).tolist() for _ in range(args.queries)]
        batches = {name: [b" ".join(word(t) for t in ws) for ws in terms]
                   for name, terms in (("zipf", zipf_terms), ("rare", rare_terms))}
        matched = {name: int(sum(df[t] for t in {t for ws in terms for t in ws}))
                   for name, terms in (("zipf", zipf_terms), ("rare", rare_terms))}

    def call(kind, qs):
        t1 = time.perf_counter()
        res = e.query(qs, args.k) if kind == "tfidf" else e.query_bm25(qs, args.k)
        wall = (time.perf_counter() - t1) * 1e3
        row = e.query_info() if kind == "tfidf" else e.bm25_info()
        row["wall_ms"] = wall
        return res, row

    def compare(qs):
        """both entry points alternately on the same run: medians, spread, allocations"""
        for _ in range(args.warmup):
            for kind in ("tfidf", "bm25"):
                call(kind, qs)
        a0 = e.alloc_counters()
        rows = {"tfidf": [], "bm25": []}
        res = {}
        for _ in range(args.reps):
            for kind in ("tfidf", "bm25"):
                res[kind], row = call(kind, qs)
                rows[kind].append(row)
        allocs = e.alloc_counters()[0] - a0[0]
        out = {"device_allocs_in_timed_calls": allocs}
        for kind in rows:
            out[kind + "_ms"] = {k: round(statistics.median(x[k] for x in rows[kind]), 4) for k in KEYS}
            out[kind + "_score_ms_min_max"] = [round(min(x["ms_score"] for x in rows[kind]), 4),
                                               round(max(x["ms_score"] for x in rows[kind]), 4)]
            out[kind + "_mean_nmatch"] = float(np.mean(res[kind]["nmatch"]))
        out["groups"] = rows["bm25"][-1]["ngroups"]
        out["distinct_terms"] = rows["bm25"][-1]["nterms"]
        s0, s1 = out["tfidf_ms"]["ms_score"], out["bm25_ms"]["ms_score"]
        out["score_ratio_bm25_over_tfidf"] = round(s1 / s0, 4) if s0 > 0 else None
        out["wall_ratio_bm25_over_tfidf"] = round(out["bm25_ms"]["wall_ms"] / out["tfidf_ms"]["wall_ms"], 4)
        return out

    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "queries": args.queries, "words_per_query": args.words, "k": args.k, "reps": args.reps, "warmup": args.warmup,
        "avgdl": None, "k1": 1.2, "b": 0.75,
    }
    for name, qs in batches.items():
        out[name] = compare(qs)
        out[name]["matched_pairs"] = matched[name]
        extra = out[name]["bm25_ms"]["ms_score"] - out[name]["tfidf_ms"]["ms_score"]
        out[name]["extra_score_ns_per_matched_pair"] = round(extra * 1e6 / matched[name], 4) if matched[name] else None
    out["avgdl"] = e.bm25_info()["avgdl"]
    out["note"] = ("device times are HIP events inside the library, medians over the timed calls, the two entry points "
                   "called alternately on one resident run; bm25 ms_lookup includes the gather of the found terms' df; "
                   "wall_ms includes host tokenising, the host's idf logs, uploads and the D2H of the rows; "
                   "matched_pairs = the sum of df over the batch's distinct words (one division each in the BM25 pass)")
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

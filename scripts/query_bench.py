#!/usr/bin/env python3
"""Top-k retrieval over a resident result (tfidf_query): config 2 generated and run on the
GPU, then a batch of 64 queries of 4 Zipf-drawn vocabulary words at k = 10.

Reports, after a warm-up, the median over --reps calls of the batch's device times (HIP
events inside the library: lookup, scoring, top-k) and host wall time; the scoring pass's
nominal bytes (12 P: every pair's term and score) over its time as a fraction of the
measured streaming-read peak (tfidf_hbm_probe); the scoring time of the 64 queries asked
one by one (64 passes) next to the batch's single pass; and tfidf_fetch of the same run,
the only other way to get at the scores.

    python3 scripts/query_bench.py [--scale S] [--commit ID] [--out profiles/query_c2.json]

With --clauses it measures tfidf_query_clauses instead, on the same run and the same queries:
tfidf_query and tfidf_query_bm25 as they are, the clause call with each query's text as its
should text (the same hits, by definition), and the clause call with the first half of each
query's tokens as must, the rest as should and one more Zipf-drawn word as must_not; the last two
under both rankings.  Per call: median and min-max over --reps of the scoring time, the top-k time
and the host wall time.

    python3 scripts/query_bench.py --clauses [--scale S] [--commit ID] [--out profiles/query_clauses_c2.json]
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
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
ap.add_argument("--clauses", action="store_true")
args = ap.parse_args()

p = tfidf_configs.plan(args.config, scale=args.scale)
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    # tfidf_fetch of the same run (every pair to the host), and the vocabulary's words
    t0 = time.perf_counter()
    with e.fetched() as r:
        fetch_s = time.perf_counter() - t0
        by_df = np.argsort(-r["term_df"].astype(np.int64), kind="stable")
        toff, tb = r["term_off"], r["term_bytes"]
        rng = np.random.default_rng(1)
        cdf = tfidf_configs.zipf_cdf(V, 1.07)     # Zipf over the words by descending document frequency
        queries = []
        for _ in range(args.queries):
            ws = by_df[np.searchsorted(cdf, rng.random(args.words))]
            queries.append(b" ".join(bytes(tb[int(toff[t]):int(toff[t + 1])]) for t in ws.tolist()))
        extra = by_df[np.searchsorted(cdf, rng.random(args.queries))]      # --clauses: one must_not word per query
        excluded = [bytes(tb[int(toff[t]):int(toff[t + 1])]) for t in extra.tolist()]

    def clause_modes():
        """name -> (call, its info): the plain calls, then the clause call in the shapes above"""
        half = [q.split() for q in queries]
        must = [b" ".join(w[:len(w) // 2]) for w in half]
        rest = [b" ".join(w[len(w) // 2:]) for w in half]
        modes = {
            "query": (lambda: e.query(queries, args.k), e.query_info),
            "query_bm25": (lambda: e.query_bm25(queries, args.k), e.bm25_info),
        }
        for name, bm in (("", None), ("_bm25", True)):
            modes["clauses_should_only" + name] = (
                lambda bm=bm: e.query_clauses(should=queries, k=args.k, bm25=bm), e.clause_info)
            modes["clauses_half_must_one_not" + name] = (
                lambda bm=bm: e.query_clauses(must, rest, excluded, args.k, None, bm), e.clause_info)
        return modes

    def measure(call, info, reps):
        rows = []
        for _ in range(reps):
            t1 = time.perf_counter()
            res = call()
            wall = (time.perf_counter() - t1) * 1e3
            row = info()
            row["wall_ms"] = wall
            rows.append(row)
        return res, rows

    if args.clauses:
        out = {"commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
               "queries": args.queries, "words_per_query": args.words, "k": args.k, "reps": args.reps, "modes": {}}
        for name, (call, info) in clause_modes().items():
            measure(call, info, 2)                 # warm-up: code objects, the context's buffers
            res, rows = measure(call, info, args.reps)
            m = {"groups": rows[-1]["ngroups"], "mean_nmatch": float(np.mean(res["nmatch"])),
                 "mean_nhits": float(np.mean(res["nhits"])),
                 "nq_unsatisfiable": rows[-1].get("nq_unsatisfiable"), "groups_tab_lds": rows[-1].get("ngroups_tab_lds")}
            for k in ("ms_score", "ms_topk", "wall_ms"):
                v = [x[k] for x in rows]
                m[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            out["modes"][name] = m
        out["note"] = ("device times are HIP events inside the calls; wall_ms includes host tokenising, uploads and "
                       "the D2H of the rows")
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        sys.exit(0)
    probe = e.hbm_probe(1 << 30, 5)

    def timed(qs, reps):
        rows = []
        for _ in range(reps):
            t1 = time.perf_counter()
            res = e.query(qs, args.k)
            wall = (time.perf_counter() - t1) * 1e3
            qi = e.query_info()
            qi["wall_ms"] = wall
            rows.append(qi)
        return res, rows

    timed(queries, 2)                              # warm-up: code objects, the context's buffers
    a0 = e.alloc_counters()
    res, rows = timed(queries, args.reps)
    allocs = e.alloc_counters()[0] - a0[0]
    med = {k: statistics.median(x[k] for x in rows) for k in ("ms_lookup", "ms_score", "ms_topk", "ms_total", "wall_ms")}
    timed(queries[:1], 2)
    single_score, single_total = 0.0, 0.0
    for q in queries:                              # the same queries one by one: one pass each
        _, one = timed([q], 3)
        single_score += statistics.median(x["ms_score"] for x in one)
        single_total += statistics.median(x["wall_ms"] for x in one)
    gbps = 12.0 * P / (med["ms_score"] * 1e-3) / 1e9 if med["ms_score"] > 0 else 0.0
    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "queries": args.queries, "words_per_query": args.words, "k": args.k, "reps": args.reps,
        "groups": rows[-1]["ngroups"], "distinct_terms": rows[-1]["nterms"], "acc_bytes": rows[-1]["acc_bytes"],
        "batch_ms": {k: round(v, 4) for k, v in med.items()},
        "batch_score_ms_min_max": [round(min(x["ms_score"] for x in rows), 4), round(max(x["ms_score"] for x in rows), 4)],
        "device_allocs_in_timed_calls": allocs,
        "score_nominal_bytes": 12 * P, "score_GBps": round(gbps, 1),
        "hbm_read_peak_GBps": round(probe["read_GBps"], 1),
        "score_fraction_of_read_peak": round(gbps / probe["read_GBps"], 4) if probe["read_GBps"] > 0 else None,
        "one_by_one_score_ms_sum": round(single_score, 3), "one_by_one_wall_ms_sum": round(single_total, 3),
        "fetch_ms": round(fetch_s * 1e3, 2), "fetch_bytes": 16 * P,
        "mean_nmatch": float(np.mean(res["nmatch"])), "mean_nhits": float(np.mean(res["nhits"])),
        "note": "device times are HIP events inside tfidf_query; wall_ms includes host tokenising, "
                "uploads and the D2H of the rows; score bytes are nominal (scores of rounds without a match are not read)",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

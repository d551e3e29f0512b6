#!/usr/bin/env python3
"""Top-k similar documents over a resident result (tfidf_similar): config 2 generated and run
on the GPU, then the nearest neighbours of random documents at k = 10.

Reports, after 2 warm-up calls, the median over --reps calls of the device times (HIP events
inside the library: table, scoring, top-k) and the host wall time for
  - 64 random rows (one group, norms cached),
  - the first call after a run (the norm pass on its own),
  - the same 64 rows one call each, summed,
  - 1024 random rows (16 groups),
next to the scoring pass's nominal bytes (12 P: every pair's term and score) over its time as
a fraction of the streaming-read peak measured in the same session (tfidf_hbm_probe), and the
64-query scoring pass of profiles/query_c2.json when that file is there.

    python3 scripts/similar_bench.py [--scale S] [--commit ID] [--out profiles/similar_c2.json]
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
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--many", type=int, default=1024)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

KEYS = ("ms_norms", "ms_table", "ms_score", "ms_topk", "ms_total", "wall_ms")

p = tfidf_configs.plan(args.config, scale=args.scale)
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    rng = np.random.default_rng(1)
    ids = np.asarray(p["doc_ids"])
    rows = rng.choice(ids, size=min(args.rows, N), replace=False)
    many = rng.choice(ids, size=min(args.many, N), replace=False)
    probe = e.hbm_probe(1 << 30, 5)

    def timed(docs, reps):
        out = []
        for _ in range(reps):
            t1 = time.perf_counter()
            res = e.similar(args.k, docs)
            wall = (time.perf_counter() - t1) * 1e3
            si = e.similar_info()
            si["wall_ms"] = wall
            out.append(si)
        return res, out

    def med(rs):
        return {k: round(statistics.median(x[k] for x in rs), 4) for k in KEYS}

    _, first = timed(rows, 1)                      # the first call after the run: computes the norms
    first = first[0]
    timed(rows, 2)                                 # warm-up: code objects, the context's buffers
    a0 = e.alloc_counters()
    res, batch = timed(rows, args.reps)
    allocs = e.alloc_counters()[0] - a0[0]
    timed(rows[:1], 2)
    a1 = e.alloc_counters()
    one = {k: 0.0 for k in KEYS}
    for d in rows.tolist():                        # the same rows one by one: one scan each
        _, rs = timed([d], 3)
        m = med(rs)
        for k in KEYS:
            one[k] += m[k]
    allocs_one = e.alloc_counters()[0] - a1[0]
    timed(many, 2)
    a2 = e.alloc_counters()
    _, big = timed(many, args.reps)
    allocs_many = e.alloc_counters()[0] - a2[0]
    b = med(batch)
    gbps = 12.0 * P / (b["ms_score"] * 1e-3) / 1e9 if b["ms_score"] > 0 else 0.0
    query_ms = None
    qpath = os.path.join(REPO, "profiles", "query_c2.json")
    if os.path.exists(qpath):
        with open(qpath) as f:
            query_ms = json.loads(f.readline()).get("batch_ms", {}).get("ms_score")
    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "rows": len(rows), "k": args.k, "reps": args.reps,
        "groups": batch[-1]["ngroups"], "group_rows": batch[-1]["group_rows"], "acc_bytes": batch[-1]["acc_bytes"],
        "big_docs": batch[-1]["big_docs"], "postings": int(np.sum(res["npairs"])),
        "batch_ms": b,
        "batch_score_ms_min_max": [round(min(x["ms_score"] for x in batch), 4), round(max(x["ms_score"] for x in batch), 4)],
        "first_call_ms": {k: round(first[k], 4) for k in KEYS},
        "one_by_one_ms_sum": {k: round(v, 3) for k, v in one.items()},
        "many_rows": len(many), "many_groups": big[-1]["ngroups"], "many_ms": med(big),
        "device_allocs_in_timed_calls": allocs, "device_allocs_one_by_one": allocs_one, "device_allocs_many": allocs_many,
        "score_nominal_bytes": 12 * P, "score_GBps": round(gbps, 1),
        "hbm_read_peak_GBps": round(probe["read_GBps"], 1),
        "score_fraction_of_read_peak": round(gbps / probe["read_GBps"], 4) if probe["read_GBps"] > 0 else None,
        "query_c2_64_queries_score_ms": query_ms,
        "mean_nmatch": float(np.mean(res["nmatch"])), "mean_nnb": float(np.mean(res["nnb"])),
        "note": "device times are HIP events inside tfidf_similar; wall_ms includes the id lookup, the rows' D2H and "
                "the result's D2H; score bytes are nominal (scores of rounds without a match are not read)",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

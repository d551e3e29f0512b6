#!/usr/bin/env python3
"""Spherical k-means over a resident result (tfidf_kmeans): config 2 generated and run on the
GPU, then K = 8, 64 and 256 clusters from the default seeds, T = 10 terms per cluster, a fixed
max_iter.

Reports per K, after --warm warm-up calls, the median (with min and max) over --reps calls of
the device times per pass (HIP events inside the library: ms_assign / passes, ms_update /
updates), the top-term selection, the host wall time, the matrix bytes, the passes made and
whether the labels settled, and the device allocations in the timed calls.  Next to the assign
time stands tfidf_similar's scoring pass over the same pairs for 64 rows, measured in the same
session: the same number of lane x pair products as K = 64, with a mask lookup instead of a
dense row load.

    python3 scripts/kmeans_bench.py [--scale S] [--iter I] [--commit ID] [--out profiles/kmeans_c2.json]
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
ap.add_argument("--ks", default="8,64,256")
ap.add_argument("--iter", type=int, default=5)
ap.add_argument("--terms", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def mmm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


p = tfidf_configs.plan(args.config, scale=args.scale)
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    rows = np.random.default_rng(1).choice(np.asarray(p["doc_ids"]), size=min(64, N), replace=False)
    for _ in range(3):
        e.similar(10, rows)
    sim_score = []
    for _ in range(args.reps):
        e.similar(10, rows)
        sim_score.append(e.similar_info()["ms_score"])
    per_k = []
    for K in [int(x) for x in args.ks.split(",")]:
        for _ in range(args.warm):
            e.kmeans(K, args.iter, args.terms)
        a0 = e.alloc_counters()
        runs = []
        for _ in range(args.reps):
            t1 = time.perf_counter()
            res = e.kmeans(K, args.iter, args.terms)
            wall = (time.perf_counter() - t1) * 1e3
            ki = e.kmeans_info()
            ki["wall_ms"] = wall
            runs.append(ki)
        allocs = e.alloc_counters()[0] - a0[0]
        last = runs[-1]
        per_k.append({
            "k": K, "passes": last["passes"], "updates": last["updates"], "converged": res["converged"],
            "split": last["split"], "matrix_bytes": last["matrix_bytes"], "work_bytes": last["work_bytes"],
            "clusterable": last["clusterable"],
            "assign_ms_per_pass": mmm([r["ms_assign"] / max(r["passes"], 1) for r in runs]),
            "update_ms_per_update": mmm([r["ms_update"] / max(r["updates"], 1) for r in runs]),
            "terms_ms": mmm([r["ms_terms"] for r in runs]),
            "total_ms": mmm([r["ms_total"] for r in runs]), "wall_ms": mmm([r["wall_ms"] for r in runs]),
            "largest_cluster": int(res["size"].max()), "empty_clusters": int((res["size"] == 0).sum()),
            "assign_products_per_pass": int(P) * K,
            "device_allocs_in_timed_calls": allocs,
        })
    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "max_iter": args.iter, "nterms": args.terms, "reps": args.reps, "warmups": args.warm,
        "similar_64_rows_score_ms": mmm(sim_score), "kmeans": per_k,
        "note": "device times are HIP events inside tfidf_kmeans, summed over a call's passes and divided by their "
                "number; wall_ms includes the ids' and norms' D2H, the seed check and the result's D2H",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

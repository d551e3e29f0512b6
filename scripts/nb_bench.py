#!/usr/bin/env python3
"""Naive Bayes over a resident result (tfidf_nb_fit / tfidf_nb_predict): config 2 generated and
run on the GPU, then a fit with K = 20 classes, every document labelled `doc id mod K`, and a
prediction of every resident document, for the multinomial and the complement variant.

Reports per variant, after --warm warm-up calls, the median (with min and max) over --reps calls
of the fit's device times (HIP events inside the library: the count pass with its reductions,
the weight pass), the host time of the logarithms and their number, the fit's host wall time, the
predict kernel's device time and the predict call's wall time (with the labels' and scores' D2H),
the matrix bytes, and the device allocations in the timed calls.

    python3 scripts/nb_bench.py [--scale S] [--k K] [--commit ID] [--out profiles/nb_c2.json]
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
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def mmm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


p = tfidf_configs.plan(args.config, scale=args.scale)
K = args.k
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    ids = np.asarray(p["doc_ids"], dtype=np.uint32)
    labels = ids % np.uint32(K)
    per_variant = []
    for variant in ("multinomial", "complement"):
        params = tfidf_abi.nb_params(ids, labels, K, variant=variant)
        for _ in range(args.warm):
            e.nb_fit(None, None, K, params=params)
            e.nb_predict()
        a0 = e.alloc_counters()
        fits, preds = [], []
        for _ in range(args.reps):
            t1 = time.perf_counter()
            e.nb_fit(None, None, K, params=params)
            fit_wall = (time.perf_counter() - t1) * 1e3
            fi = e.nb_info()
            fi["wall_ms"] = fit_wall
            fits.append(fi)
            t1 = time.perf_counter()
            res = e.nb_predict()
            pred_wall = (time.perf_counter() - t1) * 1e3
            preds.append({"ms_predict": e.nb_info()["ms_predict"], "wall_ms": pred_wall})
        allocs = e.alloc_counters()[0] - a0[0]
        last = fits[-1]
        per_variant.append({
            "variant": variant, "k": K, "labelled": int(last["nlabelled"]), "matrix_bytes": last["matrix_bytes"],
            "logs": last["nlogs"], "listed_arguments": last["nlisted"],
            "fit_count_ms": mmm([r["ms_count"] for r in fits]), "fit_weights_ms": mmm([r["ms_weights"] for r in fits]),
            "fit_logs_host_ms": mmm([r["ms_logs_host"] for r in fits]), "fit_total_ms": mmm([r["ms_total"] for r in fits]),
            "fit_wall_ms": mmm([r["wall_ms"] for r in fits]),
            "predict_ms": mmm([r["ms_predict"] for r in preds]), "predict_wall_ms": mmm([r["wall_ms"] for r in preds]),
            "predict_products": int(P) * K, "classes_predicted": int(len(set(res["label"].tolist()))),
            "device_allocs_in_timed_calls": allocs,
        })
    out = {
        "commit": args.commit, "config": args.config, "scale": args.scale, "docs": N, "pairs": P, "terms": V,
        "reps": args.reps, "warmups": args.warm, "nb": per_variant,
        "note": "device times are HIP events inside tfidf_nb_fit / tfidf_nb_predict; fit_wall_ms includes the ids' "
                "upload and lookup, the host's logarithms and the tables' upload; predict_wall_ms includes the ids' "
                "and the labels' and scores' D2H",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")

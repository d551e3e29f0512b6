#!/usr/bin/env python3
"""tfidf_transform against a resident config-2 model: config 2 generated and fitted on the GPU,
then a config-2-shaped batch of about 1e4 documents, generated on the device by a second
context, scored as a device corpus.

Two batches: the plan with another seed (the generator spells its words from the seed, so
nearly every token is outside the fitted vocabulary: the resolve stage's misses) and the plan
with the fitted seed (every token in the vocabulary: the sort and pair stages at full size).
After --warmup calls, medians over --reps calls of the per-stage device times (HIP events
inside the library), the host wall time of the call, batch GB/s over the wall time and the
out-of-vocabulary share.  As a yardstick, tfidf_run of the same batch alone on the same commit
(its whole-run device time by HIP events and its wall time).

    python3 scripts/transform_bench.py [--scale S] [--batch-scale B] [--commit ID] [--out profiles/transform_c2.json]
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
ap.add_argument("--batch-scale", type=float, default=0.1)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

STAGES = ("ms_tokens", "ms_resolve", "ms_sort", "ms_pairs")


def med(xs):
    return round(statistics.median(xs), 4)


def transform_once(e, c):
    """one tfidf_transform through the C-ABI (no words cut on the host): wall ms, info"""
    rows = tfidf_abi.Rows()
    t0 = time.perf_counter()
    rc = tfidf_abi.lib().tfidf_transform(e.h, C.byref(c), C.byref(rows))
    wall = (time.perf_counter() - t0) * 1e3
    if rc:
        raise tfidf_abi.TfidfError(rc, "tfidf_transform")
    tfidf_abi.lib().tfidf_rows_free(C.byref(rows))
    info = e.transform_info()
    info["wall_ms"] = wall
    return info


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "batch_scale": args.batch_scale,
       "reps": args.reps, "warmup": args.warmup, "transform_mb": int(os.environ.get("TFIDF_TRANSFORM_MB", "512"))}
with tfidf_abi.Engine(0) as e, tfidf_abi.Engine(0) as gen:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    fit = e.info()
    out.update(fit_docs=fit["ndocs"], fit_terms=fit["nterms"], fit_bytes=fit["nbytes"], fit_run_ms=round(fit["ms_total"], 4))
    pb = tfidf_configs.plan(args.config, scale=args.batch_scale)
    for name, seed in (("other_seed", pb["seed"] + 1), ("fitted_seed", pb["seed"])):
        b = gen.synth_device(seed, pb["V"], pb["mode"], pb["cdf"], pb["doc_ids"], pb["ntok"], pb["ndocs_total"])
        for _ in range(args.warmup):
            transform_once(e, b)
        a0 = e.alloc_counters()
        rows = [transform_once(e, b) for _ in range(args.reps)]
        allocs = e.alloc_counters()[0] - a0[0]
        last = rows[-1]
        r = {"docs": last["ndocs"], "bytes": int(b.nbytes), "tokens": last["ntokens"], "pairs": last["npairs"],
             "oov_share": round(last["noov"] / max(1, last["ntokens"]), 4), "slices": last["nslices"],
             "scratch_bytes": last["scratch_bytes"], "device_allocs_in_timed_calls": allocs}
        for k in STAGES + ("ms_total", "wall_ms"):
            r[k] = med([x[k] for x in rows])
        r["device_ms"] = med([sum(x[k] for k in STAGES) for x in rows])
        r["wall_ms_min_max"] = [round(min(x["wall_ms"] for x in rows), 4), round(max(x["wall_ms"] for x in rows), 4)]
        r["batch_GBps_wall"] = round(b.nbytes / r["wall_ms"] / 1e6, 3)
        r["batch_GBps_device"] = round(b.nbytes / r["device_ms"] / 1e6, 3)
        # the yardstick: tfidf_run of the same batch alone (its own vocabulary, df and sort of the documents)
        run_dev, run_wall = [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            gen.run_corpus(b)
            w = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                run_dev.append(gen.info()["ms_total"])
                run_wall.append(w)
        r["run_same_batch_device_ms"] = med(run_dev)
        r["run_same_batch_wall_ms"] = med(run_wall)
        r["device_ratio_transform_over_run"] = round(r["device_ms"] / r["run_same_batch_device_ms"], 3)
        r["wall_ratio_transform_over_run"] = round(r["wall_ms"] / r["run_same_batch_wall_ms"], 3)
        out[name] = r
out["note"] = ("stage times are HIP events inside the library summed over the slices, medians over the timed calls; "
               "wall_ms is the host time of the whole call: the D2H of the offsets, per slice two round trips (token "
               "total, pair total) and the copies of the rows into pageable host arrays; run_same_batch is tfidf_run "
               "of the batch alone, which leaves its result in HBM and copies nothing back")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""Vocabulary pruning on the device (tfidf_prune) on a config at full size, beside the copy rate
of the same session.

The config is generated in HBM (Engine.synth_device).  For min_df = 2 and for a max_features cut
(--features, default V / 2): --warmup run -> prune sequences and then the median, min and max of
--reps of them, from the call's own HIP events (tfidf_prune_info): ms_select (range test, the
max_features sort, bitmap, new ranks), ms_terms (the term arrays) and ms_pairs (count, scan,
write, document offsets), and the call's host wall time ms_total.  Beside them the pair pass's
floor traffic 16 P + 16 P' bytes over ms_pairs in GB/s, as a fraction of tfidf_hbm_probe's copy
GB/s from this session.  Every prune is preceded by a run (a prune changes the result), whose
device time is recorded too; the timed sequences must allocate nothing.

    python3 scripts/prune_bench.py [--config c2] [--scale S] [--commit ID] [--out profiles/prune_c2.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "python"))
import tfidf_abi  # noqa: E402
import tfidf_configs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--features", type=int, default=0)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(e, c, copy_GBps, **kw):
    ms = {"ms_select": [], "ms_terms": [], "ms_pairs": [], "ms_total": [], "run_ms": []}
    for i in range(args.warmup + args.reps):
        before = e.alloc_counters()
        e.run_corpus(c)
        run_ms = e.info()["ms_total"]
        info = e.prune(**kw)
        if i >= args.warmup:
            assert e.alloc_counters() == before
            for k in ("ms_select", "ms_terms", "ms_pairs", "ms_total"):
                ms[k].append(info[k])
            ms["run_ms"].append(run_ms)
    r = {k: spread(v) for k, v in ms.items()}
    floor = 16 * (info["npairs_before"] + info["npairs_after"])
    r.update({k: info[k] for k in ("nterms_before", "nterms_after", "npairs_before", "npairs_after", "docs_emptied", "cut_df")})
    r["pairs_floor_bytes"] = floor
    if r["ms_pairs"]["median"] > 0:       # 0: the prune removed nothing and the call returned after the selection
        r["pairs_GBps"] = round(floor / r["ms_pairs"]["median"] / 1e6, 1)
        r["pairs_fraction_of_copy"] = round(r["pairs_GBps"] / copy_GBps, 3)
    return r


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup,
       "lib": os.path.basename(tfidf_abi.LIB_PATH)}
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    out.update(nbytes=int(c.nbytes), ndocs=int(c.ndocs))
    out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    copy = out["hbm_probe"]["copy_GBps"]
    out["min_df_2"] = measure(e, c, copy, min_df=2)
    print("min_df_2", json.dumps(out["min_df_2"]), file=sys.stderr, flush=True)
    M = args.features or max(1, out["min_df_2"]["nterms_before"] // 2)
    out["max_features"] = dict(measure(e, c, copy, max_features=M), M=M)
    print("max_features", json.dumps(out["max_features"]), file=sys.stderr, flush=True)
    out["hbm_probe_after"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
out["note"] = ("ms_select / ms_terms / ms_pairs: HIP events of the call (tfidf_prune_info), ms_total its host wall time; "
               "pairs_GBps = (16 P + 16 P') / ms_pairs: the floor traffic, not the bytes moved (the count pass reads out_term a "
               "second time and the write pass gathers the new ranks); hbm_probe copy moves 2 * nbytes; run_ms: the device "
               "time of the run in front of each prune")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""Weighting schemes on the device (tfidf_reweight) on a config at full size, beside the copy rate
and tfidf_similar's norm kernel of the same session.

The config is generated in HBM (Engine.synth_device).  Per scheme: --warmup run -> reweight
sequences and then the median, min and max of --reps of them, from the call's own HIP events
(tfidf_reweight_info): ms_tables (count maximum, tables, idf by rank) and ms_pairs (the pair
pass), and the call's host wall time ms_total.  Beside them the pair pass's floor traffic of 16
bytes per pair (count, term, score) over ms_pairs in GB/s, as a fraction of tfidf_hbm_probe's
copy GB/s from this session; the floor leaves out the idf gather, the document offsets and, under
a norm, nothing: the w stay in registers for documents of up to RW_KEEP pairs.  Every reweight is
preceded by a run (the scheme of a run is the reference's), whose device time is recorded too;
the timed sequences must allocate nothing.  k_sim_norms (tfidf_similar's ms_norms over the same
pairs, reference scores) is measured the same way.

    python3 scripts/reweight_bench.py [--config c2] [--scale S] [--commit ID] [--out profiles/reweight_c2.json]
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
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

SCHEMES = {"ratio_smooth_none": ("ratio", "smooth", "none"), "log_smooth_none": ("log", "smooth", "none"),
           "ratio_ref_l2": ("ratio", "ref", "l2"), "log_smooth_l2": ("log", "smooth", "l2"), "log_smooth_l1": ("log", "smooth", "l1")}


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(e, c, copy_GBps, scheme):
    ms = {"ms_tables": [], "ms_pairs": [], "ms_total": [], "run_ms": []}
    for i in range(args.warmup + args.reps):
        before = e.alloc_counters()
        e.run_corpus(c)
        run_ms = e.info()["ms_total"]
        info = e.reweight(*scheme)
        if i >= args.warmup:
            assert e.alloc_counters() == before
            for k in ("ms_tables", "ms_pairs", "ms_total"):
                ms[k].append(info[k])
            ms["run_ms"].append(run_ms)
    r = {k: spread(v) for k, v in ms.items()}
    r.update({k: info[k] for k in ("npairs", "ndocs", "zero_norm_docs", "nlogs", "max_count", "listed_counts", "big_docs")})
    r["pairs_floor_bytes"] = 16 * info["npairs"]
    r["pairs_GBps"] = round(r["pairs_floor_bytes"] / r["ms_pairs"]["median"] / 1e6, 1)
    r["pairs_fraction_of_copy"] = round(r["pairs_GBps"] / copy_GBps, 3)
    return r


def sim_norms(e, c, doc):
    ms = []
    for i in range(args.warmup + args.reps):
        e.run_corpus(c)
        e.similar(1, [doc])
        if i >= args.warmup:
            ms.append(e.similar_info()["ms_norms"])
    return spread(ms)


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup,
       "lib": os.path.basename(tfidf_abi.LIB_PATH)}
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    out.update(nbytes=int(c.nbytes), ndocs=int(c.ndocs))
    out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    copy = out["hbm_probe"]["copy_GBps"]
    for name, scheme in SCHEMES.items():
        out[name] = measure(e, c, copy, scheme)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    out["k_sim_norms_ms"] = sim_norms(e, c, int(p["doc_ids"][0]))
    out["hbm_probe_after"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
out["note"] = ("ms_tables / ms_pairs: HIP events of the call (tfidf_reweight_info), ms_total its host wall time; pairs_GBps = "
               "16 P / ms_pairs: the floor traffic (count, term, score), not the bytes moved (the idf by rank is gathered, long "
               "documents reload their w); hbm_probe copy moves 2 * nbytes; run_ms: the device time of the run in front of "
               "each reweight; k_sim_norms_ms: tfidf_similar's ms_norms over the same pairs")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

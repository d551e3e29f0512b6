#!/usr/bin/env python3
"""Near-duplicate detection over a resident result (tfidf_near_dups): config 2 generated and run
on the GPU, then H = 128, r = 4, seed 1, threshold 0.8; and the same after word 3-grams
(tfidf_ngrams 3-3) at --ngram-scale.

Reports per case the first call (which builds the h0 table) and, after --warm warm-up calls, the
median (with min and max) over --reps calls of the four stage times (HIP events inside the
library: ms_hash, ms_sig, ms_bands, ms_verify), the host wall time, ncand, nedges, the groups, the
signature and work bytes and the device allocations in the timed calls.

Two yardsticks stand beside them; neither is a gate:
  - one tfidf_similar group scan (64 rows) from profiles/similar_c2.json and the ceil(N / 64)
    scans the all-documents form of --similar takes;
  - tfidf_hbm_probe's read rate applied to the bytes the signature pass must move: 4 P of
    out_term read plus 4 N H of signatures written (the h0 gather's 8 bytes per pair hit a table
    of 8 V bytes that stays in cache at c2's 5e4 terms and are not counted).

    python3 scripts/dedup_bench.py [--scale S] [--ngram-scale S] [--commit ID] [--out profiles/dedup_c2.json]
"""
import argparse
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
ap.add_argument("--ngram-scale", type=float, default=0.25)
ap.add_argument("--hashes", type=int, default=128)
ap.add_argument("--rows", type=int, default=4)
ap.add_argument("--threshold", type=float, default=0.8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

STAGES = ("ms_hash", "ms_sig", "ms_bands", "ms_verify", "ms_total")


def mmm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(e, read_GBps):
    info = e.info()
    P, N, V = info["npairs"], info["ndocs"], info["nterms"]
    e.near_dups(args.threshold, args.hashes, args.rows, 1)
    first = e.dedup_info()
    for _ in range(args.warm):
        e.near_dups(args.threshold, args.hashes, args.rows, 1)
    a0 = e.alloc_counters()
    runs = []
    for _ in range(args.reps):
        t1 = time.perf_counter()
        res = e.near_dups(args.threshold, args.hashes, args.rows, 1)
        wall = (time.perf_counter() - t1) * 1e3
        di = e.dedup_info()
        di["wall_ms"] = wall
        runs.append(di)
    allocs = e.alloc_counters()[0] - a0[0]
    last = runs[-1]
    sig_bytes_moved = 4 * P + 4 * N * args.hashes
    sig_ms = statistics.median(r["ms_sig"] for r in runs)
    floor_ms = sig_bytes_moved / read_GBps / 1e6
    return {
        "docs": N, "pairs": P, "terms": V, "documents_with_pairs": last["clusterable"], "big_docs": last["big_docs"],
        "ncand": last["ncand"], "nedges": last["nedges"], "ngroups": last["ngroups"],
        "sig_bytes": last["sig_bytes"], "work_bytes": last["work_bytes"],
        "first_call_ms": {k: round(first[k], 4) for k in STAGES},
        "repeated_ms": {k: mmm([r[k] for r in runs]) for k in STAGES + ("wall_ms",)},
        "device_allocs_in_timed_calls": allocs,
        "signature_pass_bytes": sig_bytes_moved,
        "signature_pass_GBps": round(sig_bytes_moved / sig_ms / 1e6, 1) if sig_ms > 0 else None,
        "signature_pass_floor_ms_at_read_rate": round(floor_ms, 4),
        "signature_pass_over_floor": round(sig_ms / floor_ms, 2) if floor_ms > 0 else None,
        "hash_evaluations": P * args.hashes,
        "edges_returned": int(res["nedges"]),
    }


out = {"commit": args.commit, "config": args.config, "hashes": args.hashes, "rows": args.rows, "seed": 1,
       "threshold": args.threshold, "reps": args.reps, "warmups": args.warm}
try:
    with open(os.path.join(REPO, "profiles", "similar_c2.json")) as f:
        sim = json.loads(f.readline())
    out["similar_group_scan_ms"] = sim["batch_ms"]["ms_total"]
    out["similar_group_rows"] = sim["group_rows"]
    out["similar_docs"] = sim["docs"]
except (OSError, ValueError, KeyError):
    out["similar_group_scan_ms"] = None

p = tfidf_configs.plan(args.config, scale=args.scale)
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    e.run_corpus(c)
    out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    out["scale"] = args.scale
    out["words"] = measure(e, out["hbm_probe"]["read_GBps"])
    print("words", json.dumps(out["words"]), file=sys.stderr, flush=True)
    if out["similar_group_scan_ms"]:
        scans = -(-out["words"]["docs"] // 64)
        all_ms = scans * out["similar_group_scan_ms"]
        out["similar_all_documents_scans"] = scans
        out["similar_all_documents_ms_extrapolated"] = round(all_ms, 1)
        out["near_dups_over_one_similar_scan"] = round(out["words"]["repeated_ms"]["ms_total"]["median"] /
                                                       out["similar_group_scan_ms"], 2)

if args.ngram_scale > 0:
    p = tfidf_configs.plan(args.config, scale=args.ngram_scale)
    with tfidf_abi.Engine(0) as e:
        c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
        g = e.ngrams(c, min_n=3, max_n=3)
        e.run_corpus(g)
        e.run_corpus(g)
        out["ngram_scale"] = args.ngram_scale
        out["ngrams_3"] = measure(e, out["hbm_probe"]["read_GBps"])
        print("ngrams_3", json.dumps(out["ngrams_3"]), file=sys.stderr, flush=True)

out["note"] = ("stage times are HIP events inside tfidf_near_dups; ms_total and wall_ms are host wall times and include the "
               "offsets' D2H, the family's upload, the candidates' D2H, the division and the union-find; ms_hash is 0 in a "
               "repeated call (the h0 table is kept); signature_pass_bytes = 4 P + 4 N H; the similar figures are read "
               "from profiles/similar_c2.json (another session's measurement), the all-documents time is an extrapolation")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

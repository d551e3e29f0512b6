#!/usr/bin/env python3
"""Fuzzy term matching at a config's vocabulary: tfidf_match_terms on the device next to
tfidf_model_match_terms, its plain-C twin, on one host thread.

The config is generated and fitted on the GPU, its model exported once (the twin's input and the
vocabulary the patterns come from).  Patterns: 64 and 4096 terms drawn with a seed, each with one
or two random byte edits; E = 50; once with the `auto` budgets of the command line (by length: up
to 2 bytes 0, up to 5 bytes 1, else 2) and once with d = 2 throughout.  Per case, after --warmup
calls, medians over --reps calls of the device times of tfidf_last_match_info (HIP events): the
scan of the table per scan launch, and the (term, pattern) pairs per second of the scans; the sort +
cut and the word gather; the host wall time of the whole call.  The twin runs the first
--twin-patterns patterns of the case once; the ratio compares pairs per second, since the twin's
time for 4096 patterns at 1e7 terms is hours.  The first --check patterns' rows of the device are
compared with the twin's, field by field.

    python3 scripts/match_bench.py [--config c2] [--scale S] [--commit ID] [--out profiles/match_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "python"))
import tfidf_abi  # noqa: E402
import tfidf_configs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", default="64,4096")
ap.add_argument("--twin-patterns", type=int, default=64)
ap.add_argument("--check", type=int, default=16)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
L = tfidf_abi.lib()


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def draw(rng, toff, tbytes, n):
    """n patterns: terms of 1..62 bytes drawn from the table, one or two random edits each"""
    V = len(toff) - 1
    out = []
    while len(out) < n:
        t = int(rng.integers(0, V))
        w = bytearray(tbytes[int(toff[t]):int(toff[t + 1])].tobytes())
        if not 1 <= len(w) <= 62:
            continue
        for _ in range(1 + len(out) % 2):
            op, at, c = int(rng.integers(0, 4)), int(rng.integers(0, len(w))), int(rng.integers(ord("a"), ord("z") + 1))
            if op == 0:
                w[at] = c
            elif op == 1:
                w.insert(at, c)
            elif op == 2 and len(w) > 1:
                del w[at]
            elif op == 3 and len(w) > 1:
                at = min(at, len(w) - 2)
                w[at], w[at + 1] = w[at + 1], w[at]
        out.append(bytes(w))
    return out


def rows(t, n, k):
    """the first n patterns' rows of a filled tfidf_term_matches"""
    def arr(p, m):
        return np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0)
    woff = arr(t.word_off, n * k + 1)
    return {"nmatch": arr(t.nmatch, n), "nterms": arr(t.nterms, n), "term": arr(t.term, n * k), "dist": arr(t.dist, n * k),
            "df": arr(t.df, n * k), "word_off": woff, "words": arr(t.word_bytes, int(woff[-1]))}


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup,
       "max_expansions": 50, "cases": []}
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    e.run_corpus(c)
    m = tfidf_abi.Model()
    rc = L.tfidf_model_export(e.h, C.byref(m))
    if rc:
        raise tfidf_abi.TfidfError(rc, "tfidf_model_export")
    V = int(m.nterms)
    toff = np.ctypeslib.as_array(m.term_off, shape=(V + 1,))
    tbytes = np.ctypeslib.as_array(m.term_bytes, shape=(int(toff[V]),))
    lens = np.diff(toff.astype(np.int64))
    out.update(terms=V, term_bytes=int(toff[V]), mean_term_bytes=round(float(lens.mean()), 3), long_terms=int((lens >= 16).sum()),
               grid_cus=e.grid_cus())
    rng = np.random.default_rng(args.seed)
    for n in [int(x) for x in args.sizes.split(",")]:
        pats = draw(rng, toff, tbytes, n)
        for name in ("auto", "d2"):
            edits = [0 if len(w) <= 2 else 1 if len(w) <= 5 else 2 for w in pats] if name == "auto" else 2
            ps, keep = tfidf_abi.make_patterns(pats, max_edits=edits)
            pr = tfidf_abi.match_params(max_expansions=50)
            walls, infos = [], []
            for i in range(args.warmup + args.reps):
                t = tfidf_abi.TermMatches()
                a0 = e.alloc_counters()
                t0 = time.perf_counter()
                rc = L.tfidf_match_terms(e.h, C.byref(ps), C.byref(pr), C.byref(t))
                w = (time.perf_counter() - t0) * 1e3
                if rc:
                    raise tfidf_abi.TfidfError(rc, "tfidf_match_terms")
                if i >= args.warmup:
                    assert e.alloc_counters() == a0
                    walls.append(w)
                    infos.append(e.match_info())
                if i + 1 < args.warmup + args.reps:
                    L.tfidf_term_matches_free(C.byref(t))
            info = infos[-1]
            pairs = V * n                                               # a scan again after an overflow adds time, not pairs
            scan = [x["ms_scan"] for x in infos]
            case = {"patterns": n, "budget": name, "scans": info["ngroups"], "selections": info["nbatches"],
                    "records": info["nrecords"], "list_records": info["list_records"],
                    "matches": int(np.ctypeslib.as_array(t.nmatch, shape=(n,)).sum()),
                    "scan_ms": spread(scan), "scan_ms_per_scan": round(statistics.median(scan) / info["ngroups"], 4),
                    "device_pairs_per_s": round(pairs / (statistics.median(scan) * 1e-3), 1),
                    "select_ms": spread([x["ms_select"] for x in infos]), "words_ms": spread([x["ms_words"] for x in infos]),
                    "wall_ms": spread(walls)}
            # ---- the twin, one thread, on the case's first patterns ----
            nt = min(n, args.twin_patterns)
            ps2, keep2 = tfidf_abi.make_patterns(pats[:nt], max_edits=edits if isinstance(edits, int) else edits[:nt])
            t2 = tfidf_abi.TermMatches()
            t0 = time.perf_counter()
            rc = L.tfidf_model_match_terms(C.byref(m), C.byref(ps2), C.byref(pr), C.byref(t2))
            tw = (time.perf_counter() - t0) * 1e3
            if rc:
                raise tfidf_abi.TfidfError(rc, "tfidf_model_match_terms")
            nc = min(nt, args.check)
            a, b = rows(t, nc, 50), rows(t2, nc, 50)
            case.update(twin_patterns=nt, twin_wall_ms=round(tw, 3), twin_pairs_per_s=round(V * nt / (tw * 1e-3), 1),
                        rows_equal_twin=bool(all(np.array_equal(a[k], b[k]) for k in a)), rows_compared=nc)
            case["device_over_twin_pairs_per_s"] = round(case["device_pairs_per_s"] / case["twin_pairs_per_s"], 2)
            L.tfidf_term_matches_free(C.byref(t))
            L.tfidf_term_matches_free(C.byref(t2))
            out["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    L.tfidf_model_free(C.byref(m))
out["note"] = ("scan_ms, select_ms and words_ms are device times between HIP events, summed over a call's launches; "
               "device_pairs_per_s = terms x patterns / scan_ms (a group scanned again after an overflow costs time and adds no pairs); the twin is tfidf_model_match_terms on one host "
               "thread over the case's first twin_patterns patterns (its model check of the whole table included), so the ratio "
               "compares rates, not two times of the same work; wall_ms is the whole C-ABI call with its read-backs")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

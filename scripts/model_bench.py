#!/usr/bin/env python3
"""The portable model at a config's vocabulary: export from a fitted context, the file, import
into a context that never ran, and tfidf_transform on the importing context next to the fitted
one.

The config is generated and fitted on the GPU (context A).  After --warmup calls, medians over
--reps calls of: tfidf_model_export on A (host wall time); tfidf_model_save / tfidf_model_load
(host only); tfidf_model_import into context B (the device time of the table's clear + build by
HIP events, and the wall time of the whole call); tfidf_transform of the config-shaped batch of
scripts/transform_bench.py (the fitted seed: every token in the vocabulary) on A and on B, the
calls alternating, each with its own spread.  One transform per context is compared field by
field, scores as bits.  As a yardstick, the wall and device time of the tfidf_run that an
import replaces (the corpus is generated in HBM, so no ingest is part of it).

    python3 scripts/model_bench.py [--config c2] [--scale S] [--batch-scale B] [--commit ID] [--out profiles/model_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

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
L = tfidf_abi.lib()


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return {"median": med(xs), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn, *a):
    t0 = time.perf_counter()
    rc = fn(*a)
    ms = (time.perf_counter() - t0) * 1e3
    if rc:
        raise tfidf_abi.TfidfError(rc, fn.__name__)
    return ms


def transform_once(e, c):
    rows = tfidf_abi.Rows()
    ms = timed(L.tfidf_transform, e.h, C.byref(c), C.byref(rows))
    L.tfidf_rows_free(C.byref(rows))
    info = e.transform_info()
    return ms, sum(info[k] for k in ("ms_tokens", "ms_resolve", "ms_sort", "ms_pairs"))


def rows_of(e, c):
    """one transform's arrays (no words cut on the host)"""
    t = tfidf_abi.Rows()
    timed(L.tfidf_transform, e.h, C.byref(c), C.byref(t))
    N, P = int(t.ndocs), int(t.npairs)

    def arr(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)
    out = {"row_off": arr(t.row_off, N + 1), "doc_size": arr(t.doc_size, N), "doc_oov": arr(t.doc_oov, N),
           "term": arr(t.term, P), "count": arr(t.count, P), "df": arr(t.df, P), "score": arr(t.score, P).view(np.uint64),
           "word_off": arr(t.word_off, P), "word_len": arr(t.word_len, P)}
    L.tfidf_rows_free(C.byref(t))
    return out


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "batch_scale": args.batch_scale,
       "reps": args.reps, "warmup": args.warmup}
n = args.warmup + args.reps
with tfidf_abi.Engine(0) as a, tfidf_abi.Engine(0) as b, tfidf_abi.Engine(0) as gen:
    c = a.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    run_wall, run_dev = [], []
    for i in range(1 + 3):
        w = timed(L.tfidf_run, a.h, C.byref(c))
        if i:
            run_wall.append(w)
            run_dev.append(a.info()["ms_total"])
    fit = a.info()
    out.update(fit_docs=fit["ndocs"], fit_terms=fit["nterms"], fit_bytes=fit["nbytes"], fit_table_slots=fit["vocab_capacity"],
               fit_run_wall_ms=spread(run_wall), fit_run_device_ms=med(run_dev))
    # ---- export ----
    walls = []
    for i in range(n):
        m = tfidf_abi.Model()
        w = timed(L.tfidf_model_export, a.h, C.byref(m))
        if i >= args.warmup:
            walls.append(w)
        if i + 1 < n:
            L.tfidf_model_free(C.byref(m))
    out["export_wall_ms"] = spread(walls)
    out["model_terms"] = int(m.nterms)
    out["model_term_bytes"] = int(m.term_off[m.nterms]) if m.nterms else 0
    # ---- the file (host only) ----
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "model.bin").encode()
        sv, ld = [], []
        for i in range(n):
            w = timed(L.tfidf_model_save, C.byref(m), path)
            m2 = tfidf_abi.Model()
            w2 = timed(L.tfidf_model_load, path, C.byref(m2))
            L.tfidf_model_free(C.byref(m2))
            if i >= args.warmup:
                sv.append(w)
                ld.append(w2)
        out["file_bytes"] = os.path.getsize(path)
        out["save_wall_ms"] = spread(sv)
        out["load_wall_ms"] = spread(ld)
    # ---- import into a context that never ran ----
    first = timed(L.tfidf_model_import, b.h, C.byref(m))
    out["import_first_wall_ms"] = round(first, 4)        # with its device allocations
    walls, builds = [], []
    for i in range(n):
        a0 = b.alloc_counters()
        w = timed(L.tfidf_model_import, b.h, C.byref(m))
        assert b.alloc_counters() == a0
        if i >= args.warmup:
            walls.append(w)
            builds.append(b.model_info()["ms_build"])
    mi = b.model_info()
    out["import_wall_ms"] = spread(walls)
    out["import_build_device_ms"] = spread(builds)
    out.update(import_table_slots=mi["table_slots"], import_long_terms=mi["long_terms"])
    L.tfidf_model_free(C.byref(m))
    # ---- transform on both ----
    pb = tfidf_configs.plan(args.config, scale=args.batch_scale)
    batch = gen.synth_device(pb["seed"], pb["V"], pb["mode"], pb["cdf"], pb["doc_ids"], pb["ntok"], pb["ndocs_total"])
    ra, rb = rows_of(a, batch), rows_of(b, batch)
    out["transform_equal_bits"] = bool(all(np.array_equal(ra[k], rb[k]) for k in ra))
    out["transform_pairs"] = int(len(ra["term"]))
    out["transform_batch_bytes"] = int(batch.nbytes)
    wa, wb, da, db = [], [], [], []
    for i in range(n):
        x, dx = transform_once(a, batch)
        y, dy = transform_once(b, batch)
        if i >= args.warmup:
            wa.append(x), wb.append(y), da.append(dx), db.append(dy)
    out["transform_fitted_wall_ms"] = spread(wa)
    out["transform_imported_wall_ms"] = spread(wb)
    out["transform_fitted_device_ms"] = spread(da)
    out["transform_imported_device_ms"] = spread(db)
out["note"] = ("wall times are host times of the whole C-ABI call; import_build_device_ms is the clear of the table "
               "and the build kernel between two HIP events; the import's wall time also holds the host check, the "
               "uploads, the idf table on the host's libm and its upload; fit_run is tfidf_run of the corpus the "
               "model came from, generated in HBM: reading a corpus from files is not part of it")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

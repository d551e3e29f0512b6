#!/usr/bin/env python3
"""Word n-grams on the device (tfidf_ngrams) on a config at full size, beside the copy rate of
the same session and the run that follows it.

The config is generated in HBM (Engine.synth_device).  For every range of --ranges, --warmup calls
and then the median, min and max of --reps calls, from the call's own HIP events
(tfidf_ngram_info): ms_bounds (token bounds, with the round trip for the token total), ms_sizes
(segment sizes, their scan and the round trip for the output's size, document offsets, tile index)
and ms_write (the write kernel).  Beside each: (input + output bytes) / ms in GB/s for the write
kernel alone and for the three stages together, as a fraction of tfidf_hbm_probe's copy GB/s from
this session, and, unless --stage-only, the K1 (tokenize+count) and whole-run ms, V and the share
of terms of >= 16 bytes of a run of the output, against the same of the corpus as generated.
A run that fails is recorded with its error, not hidden.

    python3 scripts/ngram_bench.py [--config c2] [--scale S] [--commit ID] [--out profiles/ngram_c2.json]

The A/B of the write kernel's two forms: the same script with --stage-only on the default library
and on the variant built by `make variant NAME=ngtok DEFS=-DNG_WRITE_BY_TOKEN` (TFIDF_LIB=ngtok:
one lane per token, byte stores); head_crc32 must agree between the two.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import zlib

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
ap.add_argument("--ranges", default="1-1,1-2,1-3")
ap.add_argument("--stage-only", action="store_true")
ap.add_argument("--sample", type=int, default=4 << 20)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_stats(e, c):
    """two runs of the corpus c; the second one's K1 and whole-run ms, V, and the share of terms
    of >= 16 bytes from the exported term offsets"""
    try:
        e.run_corpus(c)
        e.run_corpus(c)
        r = e.info()
        out = {"run_k1_ms": round(r["ms_tokcount"], 4), "run_ms": round(r["ms_total"], 4), "run_tokens": r["ntokens"],
               "run_terms": r["nterms"], "run_pairs": r["npairs"], "vocab_capacity": r["vocab_capacity"], "run_flags": r["flags"]}
        m = tfidf_abi.Model()
        tfidf_abi._chk(tfidf_abi.lib().tfidf_model_export(e.h, C.byref(m)), "tfidf_model_export")
        try:
            V = int(m.nterms)
            lens = np.diff(np.ctypeslib.as_array(m.term_off, shape=(V + 1,))) if V else np.zeros(0, dtype=np.uint64)
            out["terms_ge16_share"] = round(float((lens >= 16).mean()), 4) if V else 0.0
            out["term_bytes_mean"] = round(float(lens.mean()), 2) if V else 0.0
        finally:
            tfidf_abi.lib().tfidf_model_free(C.byref(m))
        return out
    except tfidf_abi.TfidfError as ex:
        return {"run_error": str(ex)}


def head_crc(e, o):
    head = tfidf_abi.Corpus()
    head.bytes, head.nbytes, head.doc_off, head.ndocs = o.bytes, min(int(o.nbytes), args.sample), o.doc_off, 0
    return zlib.crc32(bytes(e.corpus_bytes(head)[0]))


def measure(e, c, lo, hi, copy_GBps):
    ms = {"ms_bounds": [], "ms_sizes": [], "ms_write": []}
    for i in range(args.warmup + args.reps):
        before = e.alloc_counters()
        o = e.ngrams(c, min_n=lo, max_n=hi)
        if i:
            assert e.alloc_counters() == before
        if i >= args.warmup:
            info = e.ngram_info()
            for k in ms:
                ms[k].append(info[k])
    info = e.ngram_info()
    r = {k: spread(v) for k, v in ms.items()}
    moved = info["nbytes_in"] + info["nbytes_out"]
    stages = sum(r[k]["median"] for k in ms)
    r.update(nbytes_out=info["nbytes_out"], ntokens=info["ntokens"], ngrams=info["ngrams"], tile_bytes=info["tile_bytes"],
             grid=info["grid"], scratch_bytes=info["scratch_bytes"], ms_total_last=round(info["ms_total"], 4),
             write_GBps=round(moved / r["ms_write"]["median"] / 1e6, 1), stages_GBps=round(moved / stages / 1e6, 1),
             head_crc32=head_crc(e, o))
    r["write_fraction_of_copy"] = round(r["write_GBps"] / copy_GBps, 3)
    r["stages_fraction_of_copy"] = round(r["stages_GBps"] / copy_GBps, 3)
    if not args.stage_only:
        r.update(run_stats(e, o))
    return r


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup,
       "lib": os.path.basename(tfidf_abi.LIB_PATH)}
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    out.update(nbytes=int(c.nbytes), ndocs=int(c.ndocs))
    if not args.stage_only:
        out["plain"] = run_stats(e, c)
    out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    for spec in args.ranges.split(","):
        lo, hi = (int(x) for x in spec.split("-"))
        out[spec] = measure(e, c, lo, hi, out["hbm_probe"]["copy_GBps"])
        print(spec, json.dumps(out[spec]), file=sys.stderr, flush=True)
    out["hbm_probe_after"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
out["note"] = ("ms_*: HIP events of the call (tfidf_ngram_info); write_GBps = (nbytes + nbytes_out) / ms_write, stages_GBps the "
               "same over the three stages' medians; hbm_probe copy moves 2 * nbytes; run_*: the second of two runs of the "
               "shingled corpus, plain: of the corpus as generated")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

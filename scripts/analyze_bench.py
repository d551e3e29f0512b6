#!/usr/bin/env python3
"""The device analyzer (tfidf_analyze) on a config at full size, beside the copy rate of the same
session and the tokenize+count kernel it stands in front of.

The config is generated in HBM (Engine.synth_device).  Three cases, each --warmup calls and then
the median, min and max of --reps calls, from the call's own HIP events (tfidf_analyze_info's
ms_kernel: the document-start bitmap and the kernel):
  map     LOWER | PUNCT alone: the pure byte map
  filter  LOWER | PUNCT, min_len = 2 and the 318 highest-df terms of the corpus's own run as the
          stop list: the tile kernel with the table in LDS
  stem    the filter case with the Porter stemmer: the tile kernel's stemming instantiation.
          stem_share: of the tokens in the first --sample bytes of the filter case's output, the
          share that is eligible (3..64 letters a..z) and the share the stemmer changes
          (tfidf_stem_porter on the host); stemmed_tokens is the device's count over the corpus
Beside each: 2 * nbytes / ms in GB/s, tfidf_hbm_probe's copy GB/s (2 x nbytes moved as well) and
the K1 (tokenize+count) ms of a run of the analyzed corpus, all from this session.

    python3 scripts/analyze_bench.py [--config c2] [--scale S] [--commit ID] [--out profiles/analyze_c2.json]
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
ap.add_argument("--nstop", type=int, default=318)
ap.add_argument("--sample", type=int, default=2 << 20)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(e, c, **kw):
    ms = []
    for i in range(args.warmup + args.reps):
        before = e.alloc_counters()
        o = e.analyze(c, **kw)
        if i:
            assert e.alloc_counters() == before
        if i >= args.warmup:
            ms.append(e.analyze_info()["ms_kernel"])
    info = e.analyze_info()
    e.run_corpus(o)
    e.run_corpus(o)
    run = e.info()
    s = spread(ms)
    return {"ms_kernel": s, "GBps": round(2 * info["nbytes"] / s["median"] / 1e6, 1), "nstop": info["nstop"],
            "table_slots": info["table_slots"], "lds_bytes": info["lds_bytes"], "tile_bytes": info["tile_bytes"],
            "grid": info["grid"], "blanked_tokens": info["blanked_tokens"], "stemmed_tokens": info["stemmed_tokens"], "ms_total_last": round(info["ms_total"], 4),
            "run_k1_ms": round(run["ms_tokcount"], 4), "run_ms": round(run["ms_total"], 4), "run_tokens": run["ntokens"],
            "run_terms": run["nterms"]}


def stem_share(e, o):
    head = tfidf_abi.Corpus()
    head.bytes, head.nbytes, head.doc_off, head.ndocs = o.bytes, min(int(o.nbytes), args.sample), o.doc_off, 0
    toks = bytes(e.corpus_bytes(head)[0]).split()[:-1]   # the last one may be cut
    stems = {t: tfidf_abi.stem_porter(t) for t in set(toks)}
    eligible = sum(1 for t in toks if 3 <= len(t) <= tfidf_abi.AN_MAX_WORD and t.isalpha() and t.islower() and t.isascii())
    changed = sum(1 for t in toks if stems[t] != t)
    return {"sample_bytes": int(head.nbytes), "tokens": len(toks), "distinct": len(stems),
            "eligible": round(eligible / max(len(toks), 1), 4), "changed": round(changed / max(len(toks), 1), 4)}


p = tfidf_configs.plan(args.config, scale=args.scale)
out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup}
with tfidf_abi.Engine(0) as e:
    c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
    out.update(nbytes=int(c.nbytes), ndocs=int(c.ndocs))
    e.run_corpus(c)
    e.run_corpus(c)
    out["plain_run_k1_ms"] = round(e.info()["ms_tokcount"], 4)
    out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    out["map"] = measure(e, c, lower=True, punct=True)
    m = e.model_export()   # of the analyzed corpus's run
    order = sorted(range(len(m["terms"])), key=lambda t: (-int(m["df"][t]), m["terms"][t]))
    stop = [m["terms"][t] for t in order if 0 < len(m["terms"][t]) <= tfidf_abi.AN_MAX_WORD][:args.nstop]
    out["stop_bytes"] = sum(len(w) for w in stop)
    out["filter"] = measure(e, c, lower=True, punct=True, min_len=2, stop=stop)
    out["stem_share"] = stem_share(e, e.analyze(c, lower=True, punct=True, min_len=2, stop=stop))
    out["stem"] = measure(e, c, lower=True, punct=True, min_len=2, stop=stop, stem=True)
    out["filter_again"] = measure(e, c, lower=True, punct=True, min_len=2, stop=stop)["ms_kernel"]
    out["hbm_probe_after"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
for k in ("map", "filter", "stem"):
    out[k]["fraction_of_copy"] = round(out[k]["GBps"] / out["hbm_probe"]["copy_GBps"], 3)
out["note"] = ("ms_kernel: HIP events around the document-start bitmap (filter only) and the kernel; GBps = 2 * nbytes / "
               "median; hbm_probe copy moves 2 * nbytes as well; run_k1_ms is the tokenize+count kernel of a run of the "
               "analyzed corpus, plain_run_k1_ms of the corpus as generated; filter_again is the filter case measured "
               "once more behind the stem case")
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

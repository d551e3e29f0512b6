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

With --utf8 the cases of TFIDF_AN_UTF8 instead, same method:
  ab        on the config's all-ASCII corpus, the map and the filter case with the flag clear and
            with it set, in alternating calls: the cost of the flag where no byte is a sequence.
            The yardstick is the flag-clear calls' own min..max.  --ab-out FILE: the table as text
  cyrillic  about --cyr-bytes bytes of the corpus's head with every letter translated to a
            two-byte Cyrillic capital on the host, uploaded as a device corpus of documents of
            9973 bytes; LOWER | PUNCT | UTF8 in both forms (the filter case's stop list: the
            --nstop most frequent tokens of the folded head): the rate when every letter is a
            sequence

    python3 scripts/analyze_bench.py --utf8 [--out profiles/utf8_c2.json] [--ab-out profiles/utf8_ab.txt]
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
ap.add_argument("--utf8", action="store_true")
ap.add_argument("--ab-out", default="")
ap.add_argument("--cyr-bytes", type=int, default=64 << 20)
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


def alternate(e, c, **kw):
    """flag-clear and flag-set calls in turn: the same warm-ups and repetitions for each"""
    ms, changed = {False: [], True: []}, 0
    for i in range(args.warmup + args.reps):
        for u in (False, True):
            e.analyze(c, utf8=u, **kw)
            info = e.analyze_info()
            if i >= args.warmup:
                ms[u].append(info["ms_kernel"])
            changed += info["utf8_changed"]
    r = {"clear": spread(ms[False]), "utf8": spread(ms[True]), "clear_ms": [round(x, 4) for x in ms[False]],
         "utf8_ms": [round(x, 4) for x in ms[True]], "utf8_changed": changed, "lds_bytes": info["lds_bytes"], "grid": info["grid"]}
    r["delta_ms"] = round(r["utf8"]["median"] - r["clear"]["median"], 4)
    r["clear_spread_ms"] = round(r["clear"]["max"] - r["clear"]["min"], 4)
    return r


def cyrillic_head(e, c):
    """the corpus's first bytes with a..z and A..Z as U+0410..U+0429: (bytes, offsets)"""
    import numpy as np
    head = tfidf_abi.Corpus()
    head.bytes, head.nbytes, head.doc_off, head.ndocs = c.bytes, min(int(c.nbytes), args.cyr_bytes // 2 + args.cyr_bytes // 8), c.doc_off, 0
    raw = e.corpus_bytes(head)[0]
    low = raw | 0x20
    letter = (low >= 0x61) & (low <= 0x7A) & (raw < 0x80)
    n = 1 + letter.astype(np.int64)
    pos = np.cumsum(n) - n
    keep = int(np.searchsorted(pos, args.cyr_bytes))     # source bytes that fit
    raw, low, letter, pos = raw[:keep], low[:keep], letter[:keep], pos[:keep]
    total = int(pos[-1] + 1 + letter[-1])
    data = np.empty(total, dtype=np.uint8)
    data[pos[~letter]] = raw[~letter]
    data[pos[letter]] = 0xD0
    data[pos[letter] + 1] = 0x90 + (low[letter] - 0x61)
    off = np.append(np.arange(0, total, 9973, dtype=np.uint64), np.uint64(total))
    return data, off, float(letter.mean())


def measure_only(e, c, **kw):
    ms = []
    for i in range(args.warmup + args.reps):
        e.analyze(c, **kw)
        if i >= args.warmup:
            ms.append(e.analyze_info()["ms_kernel"])
    info, s = e.analyze_info(), spread(ms)
    return {"ms_kernel": s, "GBps": round(2 * info["nbytes"] / s["median"] / 1e6, 1), "utf8_changed": info["utf8_changed"],
            "blanked_tokens": info["blanked_tokens"], "lds_bytes": info["lds_bytes"], "grid": info["grid"], "nstop": info["nstop"]}


def utf8_cases():
    import collections
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import device_corpus
    p = tfidf_configs.plan(args.config, scale=args.scale)
    out = {"commit": args.commit, "config": args.config, "scale": args.scale, "reps": args.reps, "warmup": args.warmup}
    with tfidf_abi.Engine(0) as e:
        c = e.synth_device(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"], p["ndocs_total"])
        out.update(nbytes=int(c.nbytes), ndocs=int(c.ndocs))
        out["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
        e.run_corpus(e.analyze(c, lower=True, punct=True))
        m = e.model_export()
        order = sorted(range(len(m["terms"])), key=lambda t: (-int(m["df"][t]), m["terms"][t]))
        stop = [m["terms"][t] for t in order if 0 < len(m["terms"][t]) <= tfidf_abi.AN_MAX_WORD][:args.nstop]
        out["ab"] = {"map": alternate(e, c, lower=True, punct=True),
                     "filter": alternate(e, c, lower=True, punct=True, min_len=2, stop=stop),
                     "stem": alternate(e, c, lower=True, punct=True, min_len=2, stop=stop, stem=True)}
        data, off, share = cyrillic_head(e, c)
        kw = dict(lower=True, punct=True, utf8=True)
        folded = bytes(tfidf_abi.analyze_host(data[:args.sample], [0, min(len(data), args.sample)], **kw)).split()[:-1]
        cstop = [w for w, _ in collections.Counter(t for t in folded if len(t) <= tfidf_abi.AN_MAX_WORD).most_common(args.nstop)]
        out["cyrillic"] = {"nbytes": len(data), "ndocs": len(off) - 1, "letter_share_of_source_bytes": round(share, 4),
                           "stop_bytes": sum(len(w) for w in cstop)}
        with device_corpus(data, off) as dc:
            out["cyrillic"]["hbm_probe"] = {k: round(v, 1) for k, v in e.hbm_probe(max(len(data), 1 << 20), 10).items()}
            out["cyrillic"]["map"] = measure_only(e, dc, **kw)
            out["cyrillic"]["filter"] = measure_only(e, dc, min_len=2, stop=cstop, **kw)
            out["cyrillic"]["map_flag_clear"] = measure_only(e, dc, lower=True, punct=True)
            out["cyrillic"]["filter_flag_clear"] = measure_only(e, dc, lower=True, punct=True, min_len=2, stop=cstop)
        for k in ("map", "filter", "map_flag_clear", "filter_flag_clear"):
            out["cyrillic"][k]["fraction_of_copy"] = round(out["cyrillic"][k]["GBps"] / out["cyrillic"]["hbm_probe"]["copy_GBps"], 3)
        out["hbm_probe_after"] = {k: round(v, 1) for k, v in e.hbm_probe(max(int(c.nbytes), 1 << 20), 10).items()}
    out["note"] = ("ab: ms_kernel (HIP events around the document-start bitmap, where one is built, and the kernel) of calls "
                   "alternating between the flag clear and set on the all-ASCII corpus; cyrillic: every letter a two-byte "
                   "sequence, GBps = 2 * nbytes / median against the copy probe of the same size")
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.ab_out:
        with open(args.ab_out, "w") as f:
            f.write("TFIDF_AN_UTF8 on the all-ASCII %s corpus (%d bytes): ms_kernel, flag clear and flag set in alternating calls,\n"
                    "%d warm-ups and %d calls each; median (min..max)\n" % (args.config, out["nbytes"], args.warmup, args.reps))
            for k, r in out["ab"].items():
                f.write("%-7s clear %.4f (%.4f..%.4f)   utf8 %.4f (%.4f..%.4f)   delta %+.4f   clear spread %.4f\n" % (
                    k, r["clear"]["median"], r["clear"]["min"], r["clear"]["max"], r["utf8"]["median"], r["utf8"]["min"],
                    r["utf8"]["max"], r["delta_ms"], r["clear_spread_ms"]))
                f.write("        clear %s\n        utf8  %s\n" % (r["clear_ms"], r["utf8_ms"]))


if args.utf8:
    utf8_cases()
    sys.exit(0)

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

"""bench.py on the GPU: a plain run measures its headline line only, `--full` adds the
measurements that take runs of their own, and `--dump-outputs` writes what the timed path
computed, identically from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# c2 at 3 % (3000 documents, ~28 MB): more pairs than the dump's per-pair cap, so the pair
# arrays are sampled, and few enough documents and terms that those arrays are whole
ARGS = ["--gpus", "1", "--config", "c2", "--scale", "0.03", "--steps", "2", "--warmup", "1"]
PAIR_KEYS = ("doc", "term", "count", "docsize", "df", "score")
ROW_KEYS = ("doc_id", "doc_size", "term_df")


def _bench(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + ARGS + extra, capture_output=True,
                       text=True, timeout=300, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    names = sorted(os.listdir(d))
    assert names == sorted([f"pair_{k}.npy" for k in PAIR_KEYS] + [f"{k}.npy" for k in ROW_KEYS] + ["sizes.npy"])
    assert sum(os.path.getsize(os.path.join(d, n)) for n in names) <= 64_000_000
    out = {n[:-4]: np.load(os.path.join(d, n)) for n in names}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump_plain"))
    return _bench(["--dump-outputs", d]), _load(d)


def test_plain_run_is_the_headline_only(plain):
    line, _ = plain
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8/u32 (f64 score)"
    assert line["ms_per_step"] > 0
    # value = corpus bytes per second over the timed steps (both rounded to 4 decimals)
    gbs = line["config"]["corpus_bytes_total"] / (line["ms_per_step"] * 1e-3) / 1e9
    assert abs(line["value"] - gbs) <= 1e-3 * gbs + 1e-4
    assert line["roofline"]["k1_avg_ms"] > 0 and line["device_ms_per_step"] > 0
    for k in ("stage_ms", "stage_ms_mean", "stage_ms_max", "emit", "cpu_baseline"):
        assert line[k] is None, k
    assert line["roofline"]["measured_read_peak"] is None and line["roofline"]["measured_copy_peak"] is None


def test_dump_is_the_result_of_the_timed_path(plain, engine):
    """The dumped arrays are the tfidf_fetch result of the same corpus run in this process,
    the per-pair arrays at the dump's fixed sample positions."""
    import tfidf_abi
    import tfidf_configs
    sys.path.insert(0, REPO)
    import bench
    _, dump = plain
    p = tfidf_configs.plan("c2", scale=0.03)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    engine.run_host(data, off, p["doc_ids"], p["ndocs_total"])
    with engine.fetched() as r:
        P = r["npairs"]
        assert P > bench.DUMP_PAIR_CAP and r["ndocs"] <= bench.DUMP_ROW_CAP and r["nterms"] <= bench.DUMP_ROW_CAP
        assert dump["sizes"].tolist() == [P, r["ndocs"], r["nterms"], r["ndocs_total"]]
        idx = np.sort(np.random.default_rng(20240607).choice(P, size=bench.DUMP_PAIR_CAP, replace=False))
        for k in PAIR_KEYS:
            np.testing.assert_array_equal(dump[f"pair_{k}"], r[k][idx].astype(np.float64), err_msg=k)
        for k in ROW_KEYS:
            np.testing.assert_array_equal(dump[k], r[k].astype(np.float64), err_msg=k)


def test_full_run_adds_the_rest_and_dumps_the_same(plain, tmp_path):
    line0, dump0 = plain
    d = str(tmp_path / "dump_full")
    line = _bench(["--full", "--dump-outputs", d])
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "config"):
        assert line[k] == line0[k], k
    assert line["ms_per_step"] > 0
    assert set(line["stage_ms"]) == set(line["stage_ms_mean"]) == set(line["stage_ms_max"]) and line["stage_ms"]
    assert line["emit"]["text_bytes"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["single_thread"]["value"] > 0
    assert line["roofline"]["measured_read_peak"] > 0 and line["roofline"]["measured_copy_peak"] > 0
    dump = _load(d)
    for k in dump0:
        np.testing.assert_array_equal(dump[k], dump0[k], err_msg=k)

"""Offline windows of the matrix convolver against the same handle's batched passes and against the
form a user has without them, at B = 512: GPU time per block, between two stream events around
`--calls` calls of `--blocks` blocks after a warm-up call, of

  - the matrix handle with batched passes only (32 blocks per pass: the baseline),
  - the same handle with offline windows, one window (128 blocks) and two windows (256) per pass,
  - the same routes as O * I independent channels on a dense handle with batching on (its own offline
    windows from 128 partitions), the replicated input gathered on the device before the call and
    the outputs of each output's routes summed on the device after it,

for dense 2 x 2, 8 x 32 and 32 x 32 matrices and a banded 64 x 64 one (each output fed by 8
inputs), P in {128, 256, 512, 938}. Every variant is timed `--reps` times, the variants alternating,
so the spread of each is that of the same A/B on the same box (median, min and max are kept). The
bytes are the plans' (neo.matrix_offline_plan / neo.matrix_batch_plan), per block. hf_tbps_whole_pass
is the payload of the segment spectra over the time of the whole pass, windows, forward and inverse
transforms included: a lower bound for the MAC launch's rate on those bytes. spectra_first_call_ms
is the first call after a filter change less a steady call: the buffers' allocation and the
recomputation of the segment spectra. One process per configuration, each under its own time limit,
at most 16 CPU threads.
Run once on an MI355X:  python tools/matrix_offline_sweep.py --out profiles/matrix_offline_sweep.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B = 512
CONFIGS = [("dense", 2, 2), ("dense", 8, 32), ("dense", 32, 32), ("banded8", 64, 64)]
PARTITIONS = [128, 256, 512, 938]


def routes_of(kind, I, O):
    if kind == "dense":
        return [(o, i) for o in range(O) for i in range(I)]
    return [(o, (o + k) % I) for o in range(O) for k in range(8)]  # every output fed by 8 inputs


def child(kind, I, O, P, blocks, calls, reps):
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, os.path.join(HERE, "..", "neo-dsp_amd"))
    import neo

    routes = routes_of(kind, I, O)
    R, K = len(routes), len(routes) // O  # K routes per output, consecutive in the list
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    parts = torch.view_as_complex(torch.rand((R, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / (P * K))
    n = B * blocks
    x = torch.rand((I, n), device="cuda", generator=gen) * 2 - 1
    y = torch.empty((O, n), device="cuda")
    rin = torch.tensor([i for _, i in routes], device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    variants, meta, handles = {}, {}, {}

    def matrix(name, wpp):
        conv = neo.MatrixConvolver(I, O, B, P)
        conv.filter(parts, routes)
        conv.set_batch(True)
        if wpp:
            conv.set_offline(True, wpp)
            p = neo.matrix_offline_plan(I, O, B, P, routes=routes, windows=wpp)
            meta[name] = {"blocks_per_pass": p["blocks_per_pass"], "segments": p["segments"], "pairs": p["pairs"],
                          "bytes_per_block": p["bytes"] // p["blocks_per_pass"],
                          "cache_bytes_per_block": p["cache_bytes"] // p["blocks_per_pass"],
                          "hf_bytes": p["hf_bytes"], "xf_bytes": p["xf_bytes"]}
        else:
            p = neo.matrix_batch_plan(I, O, B, P, routes=routes)
            meta[name] = {"blocks_per_pass": 32, "splits": p["splits"], "bytes_per_block": p["bytes"] // 32}
        handles[name] = conv

        def call(conv=conv):
            conv.process_device(x.data_ptr(), n, y.data_ptr(), n, blocks, s)

        variants[name] = call

    matrix("matrix_batch", 0)
    if blocks >= 128:
        matrix("matrix_offline_wp1", 1)
    if blocks >= 256:
        matrix("matrix_offline_wp2", 2)

    rep = neo.UpolsConvolver(R, B, P)
    rep.filter(parts)
    rep.set_batch(True)
    xr = torch.empty((R, n), device="cuda")  # the replicated input, then the replicated channels' output
    meta["replicated_batch"] = {"offline_windows": bool(rep.offline_info()[0]) and blocks >= 128,
                                "blocks_per_pass": rep.batch_info()[0]}

    def replicated():
        torch.index_select(x, 0, rin, out=xr)
        rep.process_blocks_ptr(xr.data_ptr(), xr.data_ptr(), n, blocks, s)
        torch.sum(xr.view(O, K, n), dim=1, out=y)

    variants["replicated_batch"] = replicated

    def timed(call, ncalls=calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ncalls):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (ncalls * blocks)

    for call in variants.values():  # warm-up: one call each (the pass buffers, the caches)
        call()
    torch.cuda.synchronize()
    us = {name: [] for name in variants}
    for _ in range(reps):  # the variants alternate
        for name, call in variants.items():
            us[name].append(timed(call))

    flop = 8.0 * R * P * B  # per block, the direct form: a complex multiply-add per route, partition and bin
    res = {"matrix": kind, "inputs": I, "outputs": O, "block": B, "partitions": P, "routes": R, "blocks_per_call": blocks,
           "calls": calls, "reps": reps, "flop_per_block_direct": flop, "variants": {}}
    for name, v in us.items():
        med = float(np.median(v))
        e = {"us_per_block": round(med, 3), "us_half_range": round((max(v) - min(v)) / 2, 3),
             "us_min_max": [round(min(v), 3), round(max(v), 3)]}
        e.update(meta[name])
        if "hf_bytes" in e:  # read once per pass
            e["hf_tbps_whole_pass"] = round(e["hf_bytes"] / (med * e["blocks_per_pass"]) * 1e-6, 3)
        res["variants"][name] = e
    # the first call after a filter change: allocation and recomputation of the segment spectra
    last = "matrix_offline_wp2" if "matrix_offline_wp2" in handles else "matrix_offline_wp1" if "matrix_offline_wp1" in handles else ""
    if last:
        handles[last].filter(parts, routes)
        first = timed(variants[last], 1) * blocks
        res["variants"][last]["spectra_first_call_ms"] = round((first - res["variants"][last]["us_per_block"] * blocks) * 1e-3, 3)
    base = res["variants"]["matrix_batch"]
    for name in ("matrix_offline_wp1", "matrix_offline_wp2"):
        if name in res["variants"]:
            e = res["variants"][name]
            e["over_matrix_batch"] = round(e["us_per_block"] / base["us_per_block"], 4)
            e["ahead_of_matrix_batch"] = bool(base["us_per_block"] - e["us_per_block"] > base["us_half_range"] + e["us_half_range"])
            r = res["variants"]["replicated_batch"]
            e["over_replicated"] = round(e["us_per_block"] / r["us_per_block"], 4)
            e["ahead_of_replicated"] = bool(r["us_per_block"] - e["us_per_block"] > r["us_half_range"] + e["us_half_range"])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256, help="blocks per call")
    ap.add_argument("--calls", type=int, default=2, help="timed calls per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default="")
    ap.add_argument("--partitions", default=",".join(str(p) for p in PARTITIONS), help="the filter lengths to sweep")
    ap.add_argument("--configs", default="", help="indices into the configurations, e.g. 0,2 (default: all)")
    ap.add_argument("--only", default="", help="kind,I,O,P of one configuration (a child process)")
    a = ap.parse_args()
    if a.blocks < 128 or a.reps < 3:
        ap.error("at least 128 blocks per call and 3 alternating repetitions")
    if a.only:
        kind, I, O, P = a.only.split(",")
        child(kind, int(I), int(O), int(P), a.blocks, a.calls, a.reps)
        return
    out = {"block": B, "points": []}
    if a.out and os.path.exists(a.out):  # a sweep run in several parts keeps the points of the parts before
        with open(a.out) as f:
            out = json.load(f)
    configs = [CONFIGS[int(k)] for k in a.configs.split(",")] if a.configs else CONFIGS
    for kind, I, O in configs:
        for P in [int(v) for v in a.partitions.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", f"{kind},{I},{O},{P}", "--blocks", str(a.blocks),
                   "--calls", str(a.calls), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"matrix": kind, "inputs": I, "outputs": O, "partitions": P, "error": "time limit"}),
                      flush=True)
                sys.exit(1)  # nothing more on a device that may be hung
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode or not line:
                print(json.dumps({"matrix": kind, "inputs": I, "outputs": O, "partitions": P, "error": r.returncode,
                                  "stderr": r.stderr[-2000:]}), flush=True)
                sys.exit(1)  # a failed child ends the sweep
            pt = json.loads(line[0][7:])
            out["points"] = [q for q in out["points"] if (q["matrix"], q["inputs"], q["outputs"], q["partitions"]) !=
                             (kind, I, O, P)] + [pt]
            print(json.dumps(pt), flush=True)
            if a.out:  # after every point: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()

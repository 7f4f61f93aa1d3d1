"""Window levels of the matrix convolver against its block step and against the form a user had
without them, at B = 512 and one block per call: GPU time per block, between two stream events over
`--steps` back-to-back single-block calls after a warm-up, of

  - ONE matrix handle (neo.MatrixConvolver, automatic options) with levels off, and with levels on
    with the windows (32,), (8, 32) (the default) and (4, 8, 16, 32): set_levels between the timings,
    a warm-up of whole windows after each switch (the first level step primes),
  - the same routes as O * I independent channels on the default dense handle (streaming levels),
    the replicated input gathered on the device before the step and the outputs of each output's
    routes summed on the device after it (tools/matrix_sweep.py's "replicated_default"),

for that tool's matrices (dense 2 x 2, 8 x 32, 32 x 32, a banded 64 x 64 with 8 inputs per output)
and P in {64, 128, 256, 938}. Every variant is timed `--reps` times, the variants alternating; the
figure is the median, the spread half the range. Beside the times: the plan (head, levels, splits,
workgroups per part, slab and head-bank bytes), the bytes model of one block
(neo_hip_matrix_level_plan) and what the time makes of it in TB/s, and the multiply-adds of one
block (8 flops per bin, route and partition) in TF/s. One process per configuration, each under its
own time limit.
Run once on an MI355X:  python tools/matrix_levels_sweep.py --out profiles/matrix_levels_sweep.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from matrix_sweep import B, CONFIGS, routes_of  # noqa: E402

PARTITIONS = [64, 128, 256, 938]
WINDOWS = {"levels_32": (32,), "levels_8_32": (8, 32), "levels_4_8_16_32": (4, 8, 16, 32)}  # (8, 32) is the default


def child(kind, I, O, P, steps, warm, reps):
    import torch

    sys.path.insert(0, os.path.join(HERE, "..", "neo-dsp_amd"))
    import neo

    routes = routes_of(kind, I, O)
    R, K = len(routes), len(routes) // O  # K routes per output, consecutive in the list
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    parts = torch.view_as_complex(torch.rand((R, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / (P * K))
    nblk = 8
    x = torch.rand((I, B * nblk), device="cuda", generator=gen) * 2 - 1
    y = torch.empty((O, B * nblk), device="cuda")
    xr = torch.empty((R, B), device="cuda")
    yb = torch.empty((O, B), device="cuda")
    rin = torch.tensor([i for _, i in routes], device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    conv = neo.MatrixConvolver(I, O, B, P)
    conv.filter(parts, routes)

    def matrix_step(t):
        o = 4 * (t % nblk) * B
        conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], 1, s)

    dense = neo.UpolsConvolver(R, B, P)
    dense.set_batch(False)
    dense.filter(parts)
    del parts

    def replicated_step(t):
        blk = slice((t % nblk) * B, (t % nblk + 1) * B)
        torch.index_select(x[:, blk], 0, rin, out=xr)
        dense.process_blocks_ptr(xr.data_ptr(), xr.data_ptr(), B, 1, s)
        torch.sum(xr.view(O, K, B), dim=1, out=yb)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(steps):
            step(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    names = ["levels_off"] + list(WINDOWS) + ["replicated_default"]
    us = {n: [] for n in names}
    for t in range(warm):
        replicated_step(t)
    for _ in range(reps):  # the variants alternate
        for n in names:
            if n == "replicated_default":
                us[n].append(timed(replicated_step))
                continue
            if n == "levels_off":
                conv.set_levels(False)
            else:
                conv.set_levels(True, WINDOWS[n])
            for t in range(warm):  # whole windows: primed, the slabs' memory touched
                matrix_step(t)
            us[n].append(timed(matrix_step))
            li = conv.levels_info()
            assert n == "levels_off" or li["primed"] or not li["levels"]  # (no level: the ordinary step ran)

    res = {"matrix": kind, "inputs": I, "outputs": O, "block": B, "partitions": P, "routes": R, "steps": steps,
           "warmup": warm, "reps": reps, "flops_per_block": 8 * B * R * P, "variants": {}}
    for n, v in us.items():
        med = float(np.median(v))
        e = {"us": round(med, 2), "half_range": round((max(v) - min(v)) / 2, 2), "us_min_max": [round(min(v), 2), round(max(v), 2)],
             "tflops": round(8 * B * R * P / (med * 1e-6) / 1e12, 2)}
        if n == "levels_off":
            e["model_bytes"] = neo.matrix_plan(I, O, B, P, routes=routes)["bytes"]
        elif n in WINDOWS:
            p = neo.matrix_level_plan(I, O, B, P, routes=routes, windows=WINDOWS[n])
            e.update(head=p["head"], head_splits=p["head_splits"], head_out_tile=p["head_out_tile"],
                     levels=[{"window": lv["window"], "first": lv["first"], "last": lv["last"], "splits": lv["splits"],
                              "workgroups_per_part": round(lv["workgroups"] / lv["window"], 1)} for lv in p["levels"]],
                     partial_bytes=p["partial_bytes"], head_bank_bytes=p["head_bank_bytes"], model_bytes=p["bytes"],
                     filter_rows_per_route_and_block=p["head"] + sum((lv["last"] - lv["first"]) / lv["window"] for lv in p["levels"]))
        if "model_bytes" in e:
            e["model_tb_per_s"] = round(e["model_bytes"] / (med * 1e-6) / 1e12, 3)
        res["variants"][n] = e
    off = res["variants"]["levels_off"]["us"]
    for n in WINDOWS:
        res["variants"][n]["speedup_over_off"] = round(off / res["variants"][n]["us"], 3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128, help="a multiple of 32: whole windows of every level")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default="")
    ap.add_argument("--partitions", default=",".join(str(p) for p in PARTITIONS), help="the filter lengths to sweep")
    ap.add_argument("--configs", default="", help="matrices to sweep, e.g. 2x2,32x32 (default: all four)")
    ap.add_argument("--only", default="", help="kind,I,O,P of one configuration (a child process)")
    a = ap.parse_args()
    if a.steps < 64 or a.steps % 32 or a.warmup % 32 or a.warmup < 32 or a.reps < 3:
        ap.error("steps and warmup whole windows of 32 (at least 64 and 32), at least 3 alternating repetitions")
    if a.only:
        kind, I, O, P = a.only.split(",")
        child(kind, int(I), int(O), int(P), a.steps, a.warmup, a.reps)
        return
    out = {"block": B, "points": []}
    want = set(a.configs.split(",")) if a.configs else None
    for kind, I, O in CONFIGS:
        if want and f"{I}x{O}" not in want:
            continue
        for P in [int(v) for v in a.partitions.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", f"{kind},{I},{O},{P}", "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--reps", str(a.reps)]
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
            out["points"].append(pt)
            print(json.dumps(pt), flush=True)
            if a.out:  # after every point: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()

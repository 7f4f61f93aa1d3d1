"""The matrix convolver's step against the form a user has without it, at B = 512: GPU time per
block step, between two stream events over `--steps` back-to-back steps after a warm-up, of

  - the matrix step (neo.MatrixConvolver) at out_tile 1, 2 and 4, fused and not, and with the
    handle's automatic choices,
  - the same routes as O * I independent channels on a dense handle with levels = 0 (the plain
    step), with the replicated input gathered on the device before the step and the outputs of
    each output's routes summed on the device after it,
  - the same channels on the default handle (streaming levels), for P >= 64,

for dense 2 x 2, 8 x 32 and 32 x 32 matrices and a banded 64 x 64 one (each output fed by 8
inputs), P in {8, 32, 938}. Every variant is timed `--reps` times, the variants alternating, so
the spread of each is that of the same A/B on the same box. The bytes model is
neo_hip_matrix_plan's (8 B per FDL-row and filter-row load plus the block I/O); the fraction is
model bytes over time over 8 TB/s. One process per configuration, each under its own time limit.
Run once on an MI355X:  python tools/matrix_sweep.py --out profiles/matrix_sweep.json
(other filter lengths: --partitions 64,128,256 --out profiles/matrix_sweep_mid.json)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PEAK = 8.0e12  # bytes / s
B = 512
CONFIGS = [("dense", 2, 2), ("dense", 8, 32), ("dense", 32, 32), ("banded8", 64, 64)]
PARTITIONS = [8, 32, 938]


def routes_of(kind, I, O):
    if kind == "dense":
        return [(o, i) for o in range(O) for i in range(I)]
    return [(o, (o + k) % I) for o in range(O) for k in range(8)]  # every output fed by 8 inputs


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
    xr = torch.empty((R, B), device="cuda")  # the replicated input block, then the replicated channels' output
    yb = torch.empty((O, B), device="cuda")  # their sums per output
    rin = torch.tensor([i for _, i in routes], device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    variants, plans = {}, {}

    # every tile, fused and not, and the handle's own choices last
    for opts in [{"out_tile": ot, "fused": fused} for ot in (1, 2, 4) for fused in (0, 1)] + [{}]:
        conv = neo.MatrixConvolver(I, O, B, P, options=opts)
        conv.filter(parts, routes)
        name = f"matrix_ot{opts['out_tile']}_{'fused' if opts['fused'] else 'unfused'}" if opts else "matrix_auto"
        plans[name] = neo.matrix_plan(I, O, B, P, routes=routes, options=opts)

        def step(t, conv=conv):
            o = 4 * (t % nblk) * B
            conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], 1, s)

        variants[name] = step

    def replicated(options):
        conv = neo.UpolsConvolver(R, B, P, options=options)
        conv.set_batch(False)
        conv.filter(parts)

        def step(t, conv=conv):
            blk = slice((t % nblk) * B, (t % nblk + 1) * B)
            torch.index_select(x[:, blk], 0, rin, out=xr)
            conv.process_blocks_ptr(xr.data_ptr(), xr.data_ptr(), B, 1, s)
            torch.sum(xr.view(O, K, B), dim=1, out=yb)

        return step

    variants["replicated_plain"] = replicated({"levels": 0})
    if P >= 64:
        variants["replicated_default"] = replicated(None)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(steps):
            step(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    for step in variants.values():
        for t in range(warm):
            step(t)
    torch.cuda.synchronize()
    us = {n: [] for n in variants}
    for _ in range(reps):  # the variants alternate
        for n, step in variants.items():
            us[n].append(timed(step))

    res = {"matrix": kind, "inputs": I, "outputs": O, "block": B, "partitions": P, "routes": R, "steps": steps,
           "warmup": warm, "reps": reps, "plain_model_bytes_per_route": 16 * P * B, "variants": {}}
    for n, v in us.items():
        e = {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}
        if n in plans:
            p = plans[n]
            e.update(out_tile=p["out_tile"], fused=p["fused"], splits=p["splits"], tiles=len(p["tiles"]), model_bytes=p["bytes"],
                     fdl_row_loads=p["fdl_row_loads"], filter_row_loads=p["filter_row_loads"],
                     fraction_of_peak=round(p["bytes"] / (float(np.median(v)) * 1e-6) / PEAK, 4))
        else:  # the plain step's traffic on the replicated channels: 16 P B per route and the block I/O
            e.update(model_bytes=16 * P * B * R + 8 * B * R)
            e.update(fraction_of_peak=round(e["model_bytes"] / (float(np.median(v)) * 1e-6) / PEAK, 4))
        res["variants"][n] = e
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default="")
    ap.add_argument("--partitions", default=",".join(str(p) for p in PARTITIONS), help="the filter lengths to sweep")
    ap.add_argument("--only", default="", help="kind,I,O,P of one configuration (a child process)")
    a = ap.parse_args()
    if a.steps < 64 or a.reps < 3:
        ap.error("at least 64 steps and 3 alternating repetitions")
    if a.only:
        kind, I, O, P = a.only.split(",")
        child(kind, int(I), int(O), int(P), a.steps, a.warmup, a.reps)
        return
    out = {"block": B, "peak_bytes_per_s": PEAK, "points": []}
    for kind, I, O in CONFIGS:
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

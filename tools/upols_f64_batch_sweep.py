"""The double-precision convolver (neo.UpolsConvolver64) with batched passes on and off, at
  C3       1 x 512 x 188
  C4       256 x 256 x 3750
  C5shard  256 x 512 x 938
GPU time per block between two stream events over `--calls` device calls of `--blocks` blocks each
(64 = 4 passes of 16) after `--warmup` calls. Variants: off (the plain step pair per block, the code
path of before the passes existed, so the yardstick), t8 and t16 (set_batch(8 / 16)); name@W asks the
handle for split_workgroups = W. Every measurement is a process of its own under its own time limit;
the variants of a shape alternate, `--reps` rounds of them, so all see the same box in the same
minutes. Per block: the algorithmic bytes (off: the step's, neo.upols64_plan's rule; on: the pass's
over T, neo.upols64_batch_plan) over the median time as a fraction of 8 TB/s, and the MAC's FP64 FMAs
(4 C P B) over the time against AMD's published MI355X vector FP64 rate, 78.6 TFLOP/s = 39.3e12 FMA/s,
which is quoted, not measured here.
Run once on an MI355X:  python tools/upols_f64_batch_sweep.py --out profiles/upols_f64_batch_sweep.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PEAK = 8.0e12           # bytes / s
FMA_RATE = 78.6e12 / 2  # FP64 FMAs / s, AMD's published vector rate: not measured here
SHAPES = {"C3": (1, 512, 188), "C4": (256, 256, 3750), "C5shard": (256, 512, 938)}


def child(variant, shape, blocks, calls, warm):
    import torch

    sys.path.insert(0, os.path.join(REPO, "neo-dsp_amd"))
    import neo

    C, B, P = SHAPES[shape]
    kind, _, sw = variant.partition("@")
    sw = int(sw or 0)
    T = {"off": 0, "t8": 8, "t16": 16}[kind]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    parts = torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen, dtype=torch.float64) * 2 - 1) * (1.0 / P)
    x = torch.rand((C, B * blocks), device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    y = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    conv = neo.UpolsConvolver64(C, B, P, split_workgroups=sw)
    conv.filter(parts)
    del parts
    conv.set_batch(T)
    info = conv.batch_info()
    assert info["blocks_per_pass"] == (T or 1) and blocks % (T or 1) == 0
    n = x.shape[1]

    def call():
        conv.process_device(x.data_ptr(), n, y.data_ptr(), n, n=n, stream=s)

    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (calls * blocks)
    if T:
        plan = neo.upols64_batch_plan(C, B, P, "upols", sw, T)
        nbytes, splits = plan["pass_bytes"] / T, plan["splits"]
    else:
        splits = conv.info()["splits"]
        nbytes = 32 * C * P * B + 32 * C * splits * B + 32 * C * B  # step_bytes of csrc/upols_f64_plan.hpp
    assert torch.isfinite(y).all()
    conv.close()
    print(json.dumps({"us_per_block": us, "splits": splits, "bytes_per_block": nbytes, "fma_per_block": 4 * C * P * B}))


def summary(runs):
    us = [r["us_per_block"] for r in runs]
    med = statistics.median(us)
    return {"us_per_block": us, "median_us": med, "min_us": min(us), "max_us": max(us), "splits": runs[0]["splits"],
            "bytes_per_block": runs[0]["bytes_per_block"], "hbm_fraction": runs[0]["bytes_per_block"] / (med * 1e-6) / PEAK,
            "fma_per_block": runs[0]["fma_per_block"],
            "fp64_fraction_of_published_rate": runs[0]["fma_per_block"] / (med * 1e-6) / FMA_RATE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upols_f64_batch_sweep.json"))
    ap.add_argument("--blocks", type=int, default=64, help="blocks per call: at least 4 passes")
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--variants", default="off,t8,t16")
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement process")
    ap.add_argument("--child", nargs=2, metavar=("VARIANT", "SHAPE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.blocks, a.calls, a.warmup)
        return 0
    variants = a.variants.split(",")
    assert variants[0] == "off"
    res = {"blocks_per_call": a.blocks, "calls": a.calls, "warmup": a.warmup, "reps": a.reps, "peak_bytes_per_s": PEAK,
           "published_fp64_fma_per_s": FMA_RATE, "published_rate_measured_here": False, "shapes": {}}
    for shape in a.shapes.split(","):
        runs = {v: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--blocks", str(a.blocks), "--calls", str(a.calls),
                       "--warmup", str(a.warmup), "--child", v, shape]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                if r.returncode != 0:  # nothing more on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    return r.returncode or 1
                runs[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(shape, v, runs[v][-1], flush=True)
        C, B, P = SHAPES[shape]
        entry = {"channels": C, "block": B, "partitions": P}
        for v in variants:
            entry[v] = summary(runs[v])
            entry[v]["off_over_this_time"] = entry["off"]["median_us"] / entry[v]["median_us"]
        res["shapes"][shape] = entry
        with open(a.out, "w") as fo:  # after every shape: a later failure keeps what was measured
            json.dump(res, fo, indent=1)
            fo.write("\n")
    print(json.dumps({k: {v: round(e[v]["median_us"], 1) for v in variants} for k, e in res["shapes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The double-precision convolver (neo.UpolsConvolver64) in batched passes of 16 blocks and in offline
windows of 128, at
  C3       1 x 512 x 188
  C4       256 x 256 x 3750
  C5shard  256 x 512 x 938
GPU time per block between two stream events over `--calls` device calls of `--blocks` blocks each
(512 = 32 passes of 16 = 4 windows) after `--warmup` calls. Variants: t16 (set_batch(16): code this
work does not touch, so its figure, taken in the same run, stands for the commit before) and win
(set_offline(True)). Every measurement is a process of its own under its own time limit; the variants
of a shape alternate, `--reps` rounds of them, so all see the same box in the same minutes; the JSON
holds every repetition, the median and the half range. Per block: the algorithmic bytes (the pass's
over its blocks: neo.upols64_batch_plan, neo.upols64_offline_plan) over the median time as a fraction
of 8 TB/s. The win child also times k_upols64_ohf: a 128-block call right after filter() (it rebuilds
the segment spectra first) against the 128-block call after it, both between events, median of
`--ohf-reps` pairs.
The window kernel alone (k_upols64_omac) and the other launches of a pass come from a kernel trace of
one win child taken separately (tracing slows the host), merged with --kernel-stats:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/upols_f64_offline_sweep.py --child win C5shard
    python tools/upols_f64_offline_sweep.py --kernel-stats C5shard DIR/.../run_kernel_stats.csv
k_upols64_omac's bytes are pass_bytes less what launches 1, 3 and 4 move: the pair rows it loads, the
256 nseg spectrum rows and Y written.
Run once on an MI355X:  python tools/upols_f64_offline_sweep.py --out profiles/upols_f64_offline_sweep.json
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PEAK = 8.0e12  # bytes / s
SHAPES = {"C3": (1, 512, 188), "C4": (256, 256, 3750), "C5shard": (256, 512, 938)}
KERNELS = ("k_upols64_ohf", "k_upols64_bwindow", "k_upols64_omac", "k_upols64_bfinish", "k_upols64_bola")


def omac_bytes(C, B, P):
    """What k_upols64_omac moves per pass: the pair rows that are not zero, the spectra, Y written."""
    nseg = -(-P // 128)
    return 16 * C * B * (128 + min(128 * nseg, P - 1) + 256 * nseg + 128)


def child(variant, shape, blocks, calls, warm, ohf_reps):
    import torch

    sys.path.insert(0, os.path.join(REPO, "neo-dsp_amd"))
    import neo

    C, B, P = SHAPES[shape]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    parts = torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen, dtype=torch.float64) * 2 - 1) * (1.0 / P)
    x = torch.rand((C, B * blocks), device="cuda", generator=gen, dtype=torch.float64) * 2 - 1
    y = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    conv = neo.UpolsConvolver64(C, B, P)
    conv.filter(parts)
    if variant == "t16":
        conv.set_batch(16)
        assert conv.batch_info()["blocks_per_pass"] == 16 and blocks % 16 == 0
        nbytes = neo.upols64_batch_plan(C, B, P, "upols", 0, 16)["pass_bytes"] / 16
    else:
        conv.set_offline(True)
        assert conv.offline_info()["blocks_per_pass"] == 128 and blocks % 128 == 0
        nbytes = neo.upols64_offline_plan(C, B, P)["pass_bytes"] / 128
    n = x.shape[1]

    def call(k=n):
        conv.process_device(x.data_ptr(), n, y.data_ptr(), n, n=k, stream=s)

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    us = timed(call, calls) / (calls * blocks)
    assert torch.isfinite(y).all()
    out = {"us_per_block": us, "bytes_per_block": nbytes}
    if variant == "win":
        diffs = []
        for _ in range(ohf_reps):
            conv.filter(parts)  # marks the spectra stale; synchronous
            first = timed(lambda: call(128 * B))
            diffs.append(first - timed(lambda: call(128 * B)))
        out["ohf_us"] = statistics.median(diffs)
        out["ohf_us_all"] = diffs
    conv.close()
    print(json.dumps(out))


def summary(runs):
    us = [r["us_per_block"] for r in runs]
    med = statistics.median(us)
    s = {"us_per_block": us, "median_us": med, "half_range_us": (max(us) - min(us)) / 2,
         "bytes_per_block": runs[0]["bytes_per_block"], "hbm_fraction": runs[0]["bytes_per_block"] / (med * 1e-6) / PEAK,
         "tb_per_s": runs[0]["bytes_per_block"] / (med * 1e-6) / 1e12}
    if "ohf_us" in runs[0]:
        s["ohf_us"] = statistics.median(r["ohf_us"] for r in runs)
        s["ohf_us_runs"] = [r["ohf_us"] for r in runs]
    return s


def merge_kernel_stats(out, shape, path):
    """Per-kernel GPU times of a traced win child into the JSON: calls, average and minimum in us; the
    window kernel's bytes per pass over its average time."""
    res = json.load(open(out))
    C, B, P = SHAPES[shape]
    k = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    k[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                               "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    if "k_upols64_omac" in k:
        o = k["k_upols64_omac"]
        o["bytes_per_pass"] = omac_bytes(C, B, P)
        o["tb_per_s"] = o["bytes_per_pass"] / (o["average_us"] * 1e-6) / 1e12
        o["hbm_fraction"] = o["tb_per_s"] * 1e12 / PEAK
    res["shapes"][shape]["kernels"] = k
    with open(out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upols_f64_offline_sweep.json"))
    ap.add_argument("--blocks", type=int, default=512, help="blocks per call: 4 windows, 32 passes of 16")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ohf-reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement process")
    ap.add_argument("--child", nargs=2, metavar=("VARIANT", "SHAPE"))
    ap.add_argument("--kernel-stats", nargs=2, metavar=("SHAPE", "CSV"),
                    help="merge a rocprofv3 kernel_stats.csv of a win child into the existing --out and exit")
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.blocks, a.calls, a.warmup, a.ohf_reps)
        return 0
    if a.kernel_stats:
        merge_kernel_stats(a.out, *a.kernel_stats)
        return 0
    variants = ["t16", "win"]
    res = {"blocks_per_call": a.blocks, "calls": a.calls, "warmup": a.warmup, "reps": a.reps, "peak_bytes_per_s": PEAK,
           "shapes": {}}
    for shape in a.shapes.split(","):
        runs = {v: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--blocks", str(a.blocks), "--calls", str(a.calls),
                       "--warmup", str(a.warmup), "--ohf-reps", str(a.ohf_reps), "--child", v, shape]
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
        entry["win_over_t16_time"] = entry["win"]["median_us"] / entry["t16"]["median_us"]
        res["shapes"][shape] = entry
        with open(a.out, "w") as fo:  # after every shape: a later failure keeps what was measured
            json.dump(res, fo, indent=1)
            fo.write("\n")
    print(json.dumps({k: {"t16": round(e["t16"]["median_us"], 1), "win": round(e["win"]["median_us"], 1),
                          "ratio": round(e["win_over_t16_time"], 3)} for k, e in res["shapes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Setting up a sparse convolver from an impulse response and a dB threshold, on the device against
by hand, at the C5 shard (256 channels, B = 512, 10 s at 48 kHz: P = 938), threshold -40 dB,
A-weighting. Writes profiles/perceptual_setup.json ("perceptual masks"):

  1. wall time (host clock around synchronous calls, each ending in a stream synchronise) of
     SparseUpolsConvolver.set_impulse(ir, PerceptualSparsity) against the route without it, leg by
     leg: device normalize + uniform_partition -> download the spectra -> the predicate in numpy
     -> filter(parts, mask) (uploads spectra and mask);
  2. the device calls on spectra already on the device -- perceptual_mask (k_perc_max, k_perc_mask)
     and perceptual_histogram (k_perc_max, k_perc_hist) -- as wall time per call, with the bytes
     they move and the rate against the 8 TB/s peak; --kernel-stats merges per-kernel GPU times
     from a kernel trace of a --kernels-only run taken separately (tracing slows the host):
         rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
             python tools/perceptual_setup.py --kernels-only
         python tools/perceptual_setup.py --kernel-stats DIR/.../run_kernel_stats.csv
  3. the tile-density curve of the impulse response with and without A-weighting;
  4. the threshold threshold_for_tile_density(tiles, 0.02) gives for it.
Medians over --repeat runs after --warmup; min and max give the spread of the repeated point.

Bytes (n = C P (B + 1) bins): k_perc_max reads 8 n; k_perc_mask reads 8 n and writes n;
k_perc_hist reads 8 n (the weights and the [C][144] counters are noise beside them).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neo-dsp_amd"))
import neo  # noqa: E402

PEAK = 8.0e12  # bytes / s


def timed(fn, warmup, repeat):
    """fn is synchronous (its last step waits for its stream): host clock; ms median, min, max"""
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)}


def impulse(C, L, rate, decay_db, seed):
    """exponentially decaying noise, decay_db over its length, on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    env = torch.pow(10.0, -decay_db / 20.0 * torch.arange(L, device="cuda", dtype=torch.float32) / L)
    return (torch.randn((C, L), device="cuda", generator=g) * env).contiguous()


def numpy_mask(parts, weights, theta):
    """the predicate by hand, channel by channel (float32, the definition's order)"""
    mask = np.empty(parts.shape, np.bool_)
    for c in range(parts.shape[0]):
        power = parts[c].real ** 2 + parts[c].imag ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            x = power * (np.float32(1) / power.max())
            lvl = np.where(x > 0, np.maximum(np.float32(-144), np.float32(20) * np.log10(x)), np.float32(-144))
        mask[c] = lvl * np.float32(0.5) + weights > theta
    return mask


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ("k_perc_max", "k_perc_mask", "k_perc_hist", "k_sparse_rows", "k_sparse_pack", "k_partition"):
                if k in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--block", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=float, default=48000.0)
    ap.add_argument("--threshold", type=float, default=-40.0)
    ap.add_argument("--decay-db", type=float, default=80.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="only the device calls (for a kernel trace)")
    ap.add_argument("--kernel-stats", help="merge a rocprofv3 kernel_stats.csv into the existing --out and exit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "perceptual_setup.json"))
    a = ap.parse_args()
    C, B, L = a.channels, a.block, int(round(a.seconds * a.rate))
    P = neo.num_partitions(L, B)
    n = C * P * (B + 1)
    bytes_of = {"k_perc_max": 8 * n, "k_perc_mask": 9 * n, "k_perc_hist": 8 * n}
    if a.kernel_stats:
        res = json.load(open(a.out))
        ks = kernel_stats(a.kernel_stats)
        for k, v in ks.items():
            if k in bytes_of:
                v["bytes"] = bytes_of[k]
                v["bytes_per_s"] = bytes_of[k] / (v["average_us"] * 1e-6)
                v["fraction_of_8TBps"] = v["bytes_per_s"] / PEAK
        res["kernels"] = ks
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(ks, indent=1))
        return
    neo._native.require_gpu()
    sp = neo.PerceptualSparsity(a.rate, a.threshold, 0, "a")
    ir = impulse(C, L, a.rate, a.decay_db, 1)
    parts = neo.uniform_partition(neo.normalize_impulse(ir.clone()), B)
    torch.cuda.synchronize()
    res = {"shape": {"channels": C, "block": B, "partitions": P, "sample_rate": a.rate, "threshold_db": a.threshold,
                     "weighting": "a", "ir_decay_db": a.decay_db, "bins": n},
           "bytes_formula": "n = C P (B + 1); k_perc_max 8 n, k_perc_mask 8 n + n, k_perc_hist 8 n"}
    # 2. the device calls on device spectra
    calls = {"perceptual_mask": (lambda: neo.perceptual_mask(parts, sp), bytes_of["k_perc_max"] + bytes_of["k_perc_mask"]),
             "perceptual_histogram": (lambda: neo.perceptual_histogram(parts, sp),
                                      bytes_of["k_perc_max"] + bytes_of["k_perc_hist"])}
    res["device_calls"] = {}
    for name, (fn, nbytes) in calls.items():
        t = timed(fn, a.warmup, a.repeat if not a.kernels_only else 10)
        t.update(bytes=nbytes, bytes_per_s=nbytes / (t["median_ms"] * 1e-3))
        t["fraction_of_8TBps"] = t["bytes_per_s"] / PEAK
        res["device_calls"][name] = t
        print(name, t, flush=True)
    if a.kernels_only:
        return
    # 3. and 4. the density curves and the threshold for 2 % of the tiles
    res["density"] = {}
    for weighting in ("a", "none"):
        h = neo.perceptual_histogram(parts, neo.PerceptualSparsity(a.rate, a.threshold, 0, weighting))
        curve = neo.tile_density_curve(h["tiles"].sum(axis=0, keepdims=True))[0]
        res["density"][weighting] = {"kept_tile_fraction_at_0_to_minus_143_dB": [round(float(v), 6) for v in curve],
                                     "threshold_for_2_percent": neo.threshold_for_tile_density(h["tiles"], 0.02),
                                     "threshold_for_10_percent": neo.threshold_for_tile_density(h["tiles"], 0.10)}
        print(weighting, {k: round(float(curve[k]), 4) for k in (10, 20, 30, 40, 50, 60, 70, 80, 90)},
              res["density"][weighting]["threshold_for_2_percent"], flush=True)
    # 1. the whole setup: one call ...
    conv = neo.SparseUpolsConvolver(C, B, P)
    res["set_impulse_device_ir"] = timed(lambda: conv.set_impulse(ir, sp), a.warmup, a.repeat)
    info = conv.sparse_info()
    res["kept"] = dict(info, tile_fraction=info["kept_tiles"] / (C * P * (B // 16)))
    ir_host = ir.cpu().numpy()
    res["set_impulse_host_ir"] = timed(lambda: conv.set_impulse(ir_host, sp), 1, 3)
    print("set_impulse", res["set_impulse_device_ir"], res["set_impulse_host_ir"], res["kept"], flush=True)
    # ... against the route by hand, leg by leg
    weights = neo.perceptual_weights(B, sp)
    legs = {"partition_device": [], "download_spectra": [], "numpy_mask": [], "filter_upload": [], "total": []}
    for i in range(1 + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = neo.uniform_partition(neo.normalize_impulse(ir.clone()), B)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ph = p.cpu().numpy()
        t2 = time.perf_counter()
        m = numpy_mask(ph, weights, np.float32(a.threshold))
        t3 = time.perf_counter()
        conv.filter(ph, m)
        t4 = time.perf_counter()
        if i:  # the first pass warms up
            for k, v in zip(legs, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                legs[k].append(v * 1e3)
    res["by_hand"] = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
                      for k, v in legs.items()}
    res["by_hand"]["kept"] = conv.sparse_info()
    res["by_hand"]["bytes_over_pcie"] = {"spectra_down": 8 * n, "spectra_up": 8 * n, "mask_up": n}
    print("by hand", res["by_hand"], flush=True)
    conv.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""The sparse step against the dense steps over tile density, at the C5 shard (256 channels,
B = 512, P = 938): GPU time per step with the library's own event timing (set_timing /
step_times, as tools/plain_split_sweep.py) of

  - the sparse step (SparseUpolsConvolver) on filter + mask,
  - the dense plain step (levels = 0) on the same masked filter,
  - the dense default step (streaming levels) on the same masked filter,

for random tiles and for the decaying mask (column k of partition p kept iff k <= B 0.5^(p / tau),
tau chosen for the tile density), with the bytes model of DESIGN section 5.7, the fraction of
8 TB/s and the handles' device bytes. Two dense plain runs per point give the run-to-run spread.
Run once on an MI355X under a time limit:  python tools/sparse_sweep.py --out profiles/sparse_density.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neo-dsp_amd"))
import neo  # noqa: E402

PEAK = 8.0e12  # bytes / s


def step_us(conv, x, y, B, warm, steps):
    s = torch.cuda.current_stream()
    n = x.shape[1] // B
    for i in range(warm):
        o = 4 * (i % n) * B
        conv.process_blocks_ptr(x.data_ptr() + o, y.data_ptr() + o, x.shape[1], 1, s.cuda_stream)
    torch.cuda.synchronize()
    conv.step_times()
    conv.set_timing(True, every=1)
    for i in range(steps):
        o = 4 * (i % n) * B
        conv.process_blocks_ptr(x.data_ptr() + o, y.data_ptr() + o, x.shape[1], 1, s.cuda_stream)
    torch.cuda.synchronize()
    conv.set_timing(False)
    t = np.array(conv.step_times()) * 1e3
    # and without the per-step events (they cost a few microseconds each on the stream, which shows
    # in the 16-microsecond default step): the same steps back to back between two events
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        o = 4 * (i % n) * B
        conv.process_blocks_ptr(x.data_ptr() + o, y.data_ptr() + o, x.shape[1], 1, s.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return float(np.median(t)), float(t.min()), float(t.max()), e0.elapsed_time(e1) * 1e3 / steps


def tile_mask_random(C, P, B, d, gen):
    keep = torch.rand((C, P, B // 16), device="cuda", generator=gen) < d
    return expand_tiles(keep, B)


def expand_tiles(keep, B):
    """[C][P][NT] kept tiles -> [C][P][B+1] columns (columns 0 and B lie in tile 0)"""
    cols = keep.repeat_interleave(16, dim=2)
    return torch.cat([cols, keep[:, :, :1]], dim=2).contiguous()


def decaying(C, P, B, d):
    """column k of partition p kept iff k <= floor(B 0.5^(p / tau)); tau by bisection for tile density d"""
    p = np.arange(P)

    def tiles(tau):
        lim = np.floor(B * 0.5 ** (p / tau)).astype(np.int64)
        return np.minimum(B // 16, lim // 16 + 1)  # tiles 0 .. lim / 16 (column B only at p = 0: tile 0 anyway)

    if d >= 1.0:
        tau = 1e12
    else:
        lo, hi = 1e-3, 1e7
        for _ in range(80):
            mid = (lo * hi) ** 0.5
            lo, hi = (mid, hi) if tiles(mid).mean() < d * (B // 16) else (lo, mid)
        tau = hi
    lim = torch.from_numpy(np.floor(B * 0.5 ** (p / tau)).astype(np.int64)).cuda()
    k = torch.arange(B + 1, device="cuda")
    m = (k[None, :] <= lim[:, None])
    return m[None].expand(C, P, B + 1).contiguous(), tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--block", type=int, default=512)
    ap.add_argument("--partitions", type=int, default=938)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--densities", default="1,0.5,0.25,0.1,0.05,0.02")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    C, B, P = a.channels, a.block, a.partitions
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    parts = torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / P)
    x = torch.rand((C, B * 64), device="cuda", generator=gen) * 2 - 1
    y = torch.empty_like(x)

    m0 = neo.memory_info()["in_use"]
    sparse = neo.SparseUpolsConvolver(C, B, P)
    m1 = neo.memory_info()["in_use"]
    plain = neo.UpolsConvolver(C, B, P, options={"levels": 0})
    plain.set_batch(False)
    m2 = neo.memory_info()["in_use"]
    dflt = neo.UpolsConvolver(C, B, P)
    dflt.set_batch(False)
    m3 = neo.memory_info()["in_use"]
    S = sparse.splits
    fused = 2.0 * 8.0 * C * P * B < 64.0 * 1024 * 1024
    nw = max(1, B // 512)
    out = {"shape": {"channels": C, "block": B, "partitions": P, "splits": S}, "steps": a.steps, "warmup": a.warmup,
           "device_bytes": {"sparse_without_tiles": m1 - m0, "dense_plain": m2 - m1, "dense_default": m3 - m2},
           "points": []}
    for kind in ("random", "decaying"):
        for d in [float(v) for v in a.densities.split(",")]:
            if kind == "random":
                mask, tau = (torch.ones((C, P, B + 1), dtype=torch.bool, device="cuda") if d >= 1.0
                             else tile_mask_random(C, P, B, d, gen)), None
            else:
                mask, tau = decaying(C, P, B, d)
            masked = (parts * mask).contiguous()
            torch.cuda.synchronize()
            sparse.filter(parts, mask)
            info = sparse.sparse_info()
            sparse_bytes = (m1 - m0) + info["kept_tiles"] * 128  # the handle as created + the compacted tiles
            plain.filter(masked)
            dflt.filter(masked)
            t_sp = step_us(sparse, x, y, B, a.warmup, a.steps)
            t_pl = step_us(plain, x, y, B, a.warmup, a.steps)
            t_df = step_us(dflt, x, y, B, a.warmup, a.steps)
            t_pl2 = step_us(plain, x, y, B, a.warmup, a.steps)
            # bytes of one sparse step: kept tiles of the filter and of the FDL, the rows' bitmap words and
            # offsets, the inserted row, the slabs (written; read again by the tail), the block in and out
            model = (info["kept_tiles"] * 256 + C * P * (nw + 1) * 4 + C * B * 8 +
                     (0 if (fused and S == 1) else 2 * C * S * B * 8) + 2 * C * B * 4)
            dense_model = C * P * B * 16 + C * B * 8 + 2 * C * S * B * 8 + 2 * C * B * 4
            pt = {"mask": kind, "tile_density": info["kept_tiles"] / (C * P * (B // 16)), "target": d, "tau": tau,
                  "kept_tiles": info["kept_tiles"], "kept_bins": info["kept_bins"],
                  "sparse_us": round(t_sp[0], 2), "sparse_min_max_us": [round(t_sp[1], 2), round(t_sp[2], 2)],
                  "dense_plain_us": round(t_pl[0], 2), "dense_plain_again_us": round(t_pl2[0], 2),
                  "dense_default_us": round(t_df[0], 2),
                  "back_to_back_us": {"sparse": round(t_sp[3], 2), "dense_plain": round(t_pl[3], 2),
                                      "dense_default": round(t_df[3], 2)},
                  "sparse_over_dense_default_back_to_back": round(t_sp[3] / t_df[3], 4),
                  "model_bytes": model, "fraction_of_peak": round(model / (t_sp[0] * 1e-6) / PEAK, 4),
                  "dense_plain_model_bytes": dense_model,
                  "dense_plain_fraction_of_peak": round(dense_model / (t_pl[0] * 1e-6) / PEAK, 4),
                  "sparse_over_dense_plain": round(t_sp[0] / t_pl[0], 4),
                  "sparse_over_dense_default": round(t_sp[0] / t_df[0], 4),
                  "sparse_device_bytes": sparse_bytes, "sparse_filter_bytes": info["filter_bytes"]}
            out["points"].append(pt)
            print(json.dumps(pt), flush=True)
            del mask, masked
            if a.out:  # after every point: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    sparse.close()
    plain.close()
    dflt.close()


if __name__ == "__main__":
    main()

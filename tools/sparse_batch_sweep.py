"""The batched sparse pass against the one-block-per-pass sparse step and the dense batched passes
over tile density, at the C5 shard (256 channels, B = 512, P = 938): 1024 device-resident blocks
through process_blocks_ptr, time per block from an event pair around the call, of

  - the sparse handle with batching on (T blocks per k_sparse_batch_mac pass), twice,
  - the sparse handle with batching off (one k_upols_sparse_step per block), twice: the spread,
  - the dense handle on the same masked filter, batched, offline windows off and on,

for random tiles and for the decaying mask of tools/sparse_sweep.py, with the bytes model of DESIGN
section 5.7 and the fraction of 8 TB/s. One GPU process, run once under a time limit:

  python tools/sparse_batch_sweep.py --out profiles/sparse_batch_density.json

A/B against another build of the library (the parent commit's): the same masks and blocks through
that tree's package, the unbatched column only, then merged as `parent_unbatched_us`:

  python tools/sparse_batch_sweep.py --neo OTHER_TREE/neo-dsp_amd --unbatched-only --out parent.json
  python tools/sparse_batch_sweep.py --parent parent.json --out profiles/sparse_batch_density.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

PEAK = 8.0e12  # bytes / s


def per_block_us(conv, x, y, B, nblocks, warm_blocks):
    """one warm call (buffers of the first batched pass, spectra of the first offline pass), then
    the timed call of nblocks blocks between two events"""
    s = torch.cuda.current_stream()
    conv.process_blocks_ptr(x.data_ptr(), y.data_ptr(), x.shape[1], warm_blocks, s.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    conv.process_blocks_ptr(x.data_ptr(), y.data_ptr(), x.shape[1], nblocks, s.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / nblocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--block", type=int, default=512)
    ap.add_argument("--partitions", type=int, default=938)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--warm-blocks", type=int, default=256)
    ap.add_argument("--densities", default="1,0.5,0.25,0.1,0.05,0.02")
    ap.add_argument("--neo", default="", help="the neo-dsp_amd directory of another tree (its package and library)")
    ap.add_argument("--unbatched-only", action="store_true")
    ap.add_argument("--parent", default="", help="a --unbatched-only result of the parent build to merge")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    # the package under test first (this tree's unless --neo), then the mask families of
    # tools/sparse_sweep.py, whose own `import neo` finds it loaded
    sys.path.insert(0, os.path.abspath(a.neo) if a.neo else os.path.join(HERE, "..", "neo-dsp_amd"))
    import neo

    sys.path.insert(0, HERE)
    from sparse_sweep import decaying, tile_mask_random

    C, B, P, nb = a.channels, a.block, a.partitions, a.blocks
    parent = json.load(open(a.parent)) if a.parent else None
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    parts = torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / P)
    x = torch.rand((C, B * nb), device="cuda", generator=gen) * 2 - 1
    y = torch.empty_like(x)
    sparse = neo.SparseUpolsConvolver(C, B, P)
    dense = None if a.unbatched_only else neo.UpolsConvolver(C, B, P)
    nw = max(1, B // 512)
    out = {"shape": {"channels": C, "block": B, "partitions": P, "splits": sparse.splits}, "blocks": nb,
           "warm_blocks": a.warm_blocks, "library": os.path.relpath(neo._native.LIB_PATH, os.path.join(HERE, "..")), "points": []}
    if not a.unbatched_only:
        sb = sparse.sparse_batch_info()
        out["shape"].update(batch_blocks=sb["blocks_per_pass"], batch_splits=sb["splits"])
    for kind in ("random", "decaying"):
        for d in [float(v) for v in a.densities.split(",")]:
            if kind == "random":
                mask, tau = (torch.ones((C, P, B + 1), dtype=torch.bool, device="cuda") if d >= 1.0
                             else tile_mask_random(C, P, B, d, gen)), None
            else:
                mask, tau = decaying(C, P, B, d)
            torch.cuda.synchronize()
            sparse.filter(parts, mask)
            info = sparse.sparse_info()
            pt = {"mask": kind, "target": d, "tau": tau, "tile_density": info["kept_tiles"] / (C * P * (B // 16)),
                  "kept_tiles": info["kept_tiles"]}
            if not a.unbatched_only:
                sparse.set_batch(True)
                t_b = [per_block_us(sparse, x, y, B, nb, a.warm_blocks) for _ in range(2)]
                sparse.set_batch(False)
            t_u = [per_block_us(sparse, x, y, B, nb, a.warm_blocks) for _ in range(2)]
            pt["sparse_unbatched_us"] = [round(v, 3) for v in t_u]
            pt["unbatched_spread"] = round(abs(t_u[0] - t_u[1]) / min(t_u), 4)
            if not a.unbatched_only:
                masked = (parts * mask).contiguous()
                dense.filter(masked)
                del masked
                dense.set_offline(False)
                t_d = per_block_us(dense, x, y, B, nb, a.warm_blocks)
                dense.set_offline(True)
                t_o = per_block_us(dense, x, y, B, nb, a.warm_blocks)
                sbi = sparse.sparse_batch_info()
                T, Sb = sbi["blocks_per_pass"], sbi["splits"]
                # bytes of one T-block pass: kept filter tiles, FDL tiles of the window bitmaps (the T - 1
                # rows preloaded per split are of the same windows), the rows' bitmap, window and
                # offset words, and per block the inserted row (written), the slabs (written, read by
                # the finish) and the block in and out
                model = (info["kept_tiles"] * 128 + sbi["window_tiles"] * 128 + C * P * (2 * nw + 1) * 4 +
                         T * (C * B * 8 + 2 * C * Sb * B * 8 + 2 * C * B * 4))
                tb = float(np.mean(t_b))
                pt.update({"window_tiles": sbi["window_tiles"],
                           "sparse_batched_us": [round(v, 3) for v in t_b],
                           "dense_batched_us": round(t_d, 3), "dense_offline_us": round(t_o, 3),
                           "batched_over_unbatched": round(tb / float(np.mean(t_u)), 4),
                           "batched_over_dense_batched": round(tb / t_d, 4),
                           "batched_over_dense_offline": round(tb / t_o, 4),
                           "model_bytes_per_pass": model,
                           "fraction_of_peak": round(model / (tb * T * 1e-6) / PEAK, 4)})
                # the same 64 blocks from a reset handle, batched and one block per pass: another order
                # of the same sums, peak-normalized difference at the shape that is timed
                s = torch.cuda.current_stream().cuda_stream
                ys = []
                for on in (True, False):
                    sparse.reset()
                    sparse.set_batch(on)
                    sparse.process_blocks_ptr(x.data_ptr(), y.data_ptr(), x.shape[1], 64, s)
                    ys.append(y[:, : 64 * B].clone())
                pt["batched_vs_unbatched_peak_err"] = float((ys[0] - ys[1]).abs().max() / ys[1].abs().max().clamp_min(1e-30))
                del ys
                if parent:
                    pp = [q for q in parent["points"] if q["mask"] == kind and q["target"] == d]
                    if pp and pp[0]["kept_tiles"] == info["kept_tiles"]:
                        pu = pp[0]["sparse_unbatched_us"]
                        pt["parent_unbatched_us"] = pu
                        pt["parent_spread"] = pp[0]["unbatched_spread"]
                        pt["unbatched_over_parent"] = round(float(np.mean(t_u)) / float(np.mean(pu)), 4)
                        # the bar: below the parent's by more than the spread of its two runs
                        pt["batched_below_parent_by_more_than_spread"] = bool(max(t_b) < min(pu) * (1 - pp[0]["unbatched_spread"]))
            out["points"].append(pt)
            print(json.dumps(pt), flush=True)
            del mask
            if a.out:  # after every point: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    sparse.close()
    if dense is not None:
        dense.close()


if __name__ == "__main__":
    main()

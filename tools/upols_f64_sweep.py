"""The double-precision block step (neo.UpolsConvolver64: k_upols64_step + k_upols64_finish) beside the
float32 plain step (neo.UpolsConvolver with options levels 0, batch_blocks 0 and set_batch(False): the
two-launch or one-launch step over the whole filter, no streaming levels), at
  C3       1 x 512 x 188
  C4       256 x 256 x 3750
  C5shard  256 x 512 x 938
GPU time per block between two stream events over `--steps` back-to-back single-block device calls
after `--warmup` calls. Every measurement is a process of its own under its own time limit; the
float and the double processes of a shape alternate, `--reps` of each, so both see the same box in the
same minutes. --float-tree DIR (a checkout of the parent commit with its library built) takes the
float handle from there; by default it is this tree's, whose float sources this feature does not touch.
Per step: its algorithmic bytes (filter + FDL rows once, slabs written and read, the block in, the
previous block or tail in and out, the block out) over its time, as a fraction of 8 TB/s.
Run once on an MI355X:  python tools/upols_f64_sweep.py --out profiles/upols_f64_sweep.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PEAK = 8.0e12  # bytes / s
SHAPES = {"C3": (1, 512, 188), "C4": (256, 256, 3750), "C5shard": (256, 512, 938)}


def child(kind, tree, shape, steps, warm):
    import torch

    sys.path.insert(0, os.path.join(tree, "neo-dsp_amd"))
    import neo

    C, B, P = SHAPES[shape]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    f64 = kind == "double"
    real = torch.float64 if f64 else torch.float32
    parts = torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen, dtype=real) * 2 - 1) * (1.0 / P)
    nblk = 8
    x = torch.rand((C, B * nblk), device="cuda", generator=gen, dtype=real) * 2 - 1
    y = torch.empty_like(x)
    word = 8 if f64 else 4
    s = torch.cuda.current_stream().cuda_stream
    if f64:
        conv = neo.UpolsConvolver64(C, B, P)
        conv.filter(parts)
        S = conv.info()["splits"]

        def step(t):
            o = word * (t % nblk) * B
            conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], stream=s)
    else:
        conv = neo.UpolsConvolver(C, B, P, options={"levels": 0, "batch_blocks": 0})
        conv.set_batch(False)
        conv.filter(parts)
        S = conv.splits

        def step(t):
            o = word * (t % nblk) * B
            conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], s)
    del parts
    for t in range(warm):
        step(t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(steps):
        step(t)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / steps
    cw = 2 * word  # one complex value
    nbytes = 2 * cw * C * P * B + 2 * cw * C * S * B + 4 * word * C * B
    assert torch.isfinite(y).all()
    conv.close()
    print(json.dumps({"us_per_block": us, "splits": S, "bytes": nbytes}))


def summary(runs):
    us = [r["us_per_block"] for r in runs]
    med = statistics.median(us)
    return {"us_per_block": us, "median_us": med, "min_us": min(us), "max_us": max(us), "splits": runs[0]["splits"],
            "bytes": runs[0]["bytes"], "hbm_fraction": runs[0]["bytes"] / (med * 1e-6) / PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upols_f64_sweep.json"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--float-tree", default=REPO)
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement process")
    ap.add_argument("--child", nargs=3, metavar=("KIND", "TREE", "SHAPE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.steps, a.warmup)
        return 0
    res = {"steps": a.steps, "warmup": a.warmup, "reps": a.reps, "peak_bytes_per_s": PEAK,
           "float_tree": "this tree" if os.path.samefile(a.float_tree, REPO) else "parent commit", "shapes": {}}
    for shape in a.shapes.split(","):
        runs = {"float": [], "double": []}
        for _ in range(a.reps):
            for kind, tree in (("float", a.float_tree), ("double", REPO)):
                cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
                       "--child", kind, tree, shape]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                if r.returncode != 0:  # nothing more on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    return r.returncode or 1
                runs[kind].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(shape, kind, runs[kind][-1], flush=True)
        C, B, P = SHAPES[shape]
        f, d = summary(runs["float"]), summary(runs["double"])
        res["shapes"][shape] = {"channels": C, "block": B, "partitions": P, "float_plain": f, "double": d,
                                "double_over_float_time": d["median_us"] / f["median_us"],
                                "double_over_float_hbm_fraction": d["hbm_fraction"] / f["hbm_fraction"]}
        with open(a.out, "w") as fo:  # after every shape: a later failure keeps what was measured
            json.dump(res, fo, indent=1)
            fo.write("\n")
    print(json.dumps({k: {"float_us": v["float_plain"]["median_us"], "double_us": v["double"]["median_us"],
                          "float_hbm": v["float_plain"]["hbm_fraction"], "double_hbm": v["double"]["hbm_fraction"]}
                      for k, v in res["shapes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The dense convolvers' fade step (a live filter update, neo.UpolsConvolver.update_filter) beside
the steps it stands in for, at the benchmark's shapes: the C5 shard (256 x 512 x 938), C4
(256 x 256 x 1875) and C3 (1 x 512 x 188). GPU time per block, between two stream events over
`--steps` back-to-back single-block calls after a warm-up, of

  (a) fade_step    an update over `--steps` blocks on a handle with the default options, then that
                   many calls (two launches each: both banks against the same delay-line rows; two
                   inverse transforms and the mix),
  (b) plain_step   the same shape's plain step (options levels = 0): what two of stand behind a
                   fade block without the feature,
  (c) stream_step  the same shape's streaming step (the default options, batching off),
  (d) update       the update_filter call itself with a device tensor (fade_blocks = 1): host wall
                   time of the call and GPU time between two events around it,
  (e) first_after  the first block after a fade on the streaming handle: the levels primed again
                   from the stepped delay line and, with a far level, its segment spectra from B.

Every variant is timed `--reps` times, the variants alternating, so the spread of each is that of
the same A/B on the same box. One process per shape, each under its own time limit.
--parent-tree DIR (a checkout of the parent commit with its library built): (b) and (c) once more
there, in processes that alternate with this tree's, `--reps` times each: the ordinary steps' A/B.
Run once on an MI355X:  python tools/upols_fade_sweep.py --out profiles/upols_fade_sweep.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"c5": (256, 512, 938), "c4": (256, 256, 1875), "c3": (1, 512, 188)}  # channels, block, partitions


def setup(tree, C, B, P):
    import torch

    sys.path.insert(0, os.path.join(tree, "neo-dsp_amd"))
    import neo

    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    mk = lambda: torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / P)
    nblk = 8
    x = torch.rand((C, B * nblk), device="cuda", generator=gen) * 2 - 1
    y = torch.empty((C, B * nblk), device="cuda")
    return torch, neo, mk, nblk, x, y


def timed(torch, step, steps, before=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before:
        before()
        torch.cuda.synchronize()
    e0.record()
    for t in range(steps):
        step(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def stepper(conv, nblk, x, y, B, s):
    def step(t):
        o = 4 * (t % nblk) * B
        conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], s)
    return step


def child_steps(tree, C, B, P, steps, warm):
    """(b) and (c) alone, in the tree given: two figures"""
    torch, neo, mk, nblk, x, y = setup(tree, C, B, P)
    s = torch.cuda.current_stream().cuda_stream
    pa = mk()
    res = {}
    for name, options in (("plain_step", {"levels": 0}), ("stream_step", None)):
        conv = neo.UpolsConvolver(C, B, P, options=options)
        conv.filter(pa)
        conv.set_batch(False)
        step = stepper(conv, nblk, x, y, B, s)
        for t in range(warm):
            step(t)
        torch.cuda.synchronize()
        res[name] = timed(torch, step, steps)
        conv.close()
    print("RESULT " + json.dumps(res), flush=True)


def child(C, B, P, steps, warm, reps):
    torch, neo, mk, nblk, x, y = setup(os.path.join(HERE, ".."), C, B, P)
    s = torch.cuda.current_stream().cuda_stream
    banks = [mk(), mk()]

    def handle(options):
        conv = neo.UpolsConvolver(C, B, P, options=options)
        conv.filter(banks[0])
        conv.set_batch(False)
        return conv

    plain, stream, fading, upd = handle({"levels": 0}), handle(None), handle(None), handle(None)
    flip = {"n": 0}

    def arm():  # a fade over exactly the timed steps: the handle is back to its own steps after them
        flip["n"] += 1
        fading.update_filter(banks[flip["n"] % 2], fade_blocks=steps, stream=s)

    def update_times(n):
        host, gpu, first = [], [], []
        one = stepper(upd, nblk, x, y, B, s)
        for k in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            upd.update_filter(banks[(k + 1) % 2], fade_blocks=1, stream=s)
            host.append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            gpu.append(e0.elapsed_time(e1) * 1e3)
            one(k)  # the fade's one block: the next update is allowed
            torch.cuda.synchronize()
            first.append(timed(torch, lambda t: one(k + 1), 1))  # the first block after the fade
            for t in range(3):  # a few streaming steps between the updates
                one(k + 2 + t)
        return float(np.median(host)), float(np.median(gpu)), float(np.median(first))

    variants = {"fade_step": (stepper(fading, nblk, x, y, B, s), arm), "plain_step": (stepper(plain, nblk, x, y, B, s), None),
                "stream_step": (stepper(stream, nblk, x, y, B, s), None)}
    for step, before in variants.values():
        if before:
            before()
        for t in range(max(warm, steps) if before else warm):  # the warm-up fade runs to its end
            step(t)
    update_times(2)
    torch.cuda.synchronize()
    us = {n: [] for n in variants}
    up = []
    for _ in range(reps):  # the variants alternate
        for n, (step, before) in variants.items():
            us[n].append(timed(torch, step, steps, before))
        up.append(update_times(5))
    assert fading.fade_info()["remaining_blocks"] == 0
    res = {"channels": C, "block": B, "partitions": P, "steps": steps, "warmup": warm, "reps": reps,
           "plain_splits": plain.splits, "streaming": bool(stream.ahead_info()[0]),
           "bank_bytes": fading.fade_info()["bank_bytes"], "variants": {}}

    def stat(v, key="us"):
        return {key: round(float(np.median(v)), 2), key + "_min_max": [round(min(v), 2), round(max(v), 2)]}

    for n, v in us.items():
        res["variants"][n] = stat(v)
    res["variants"]["update"] = {**stat([h for h, _, _ in up], "host_us"), **stat([q for _, q, _ in up], "gpu_us")}
    res["variants"]["first_after"] = stat([f for _, _, f in up])
    res["fade_over_plain"] = round(res["variants"]["fade_step"]["us"] / res["variants"]["plain_step"]["us"], 3)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"args": args, "error": "time limit"}), flush=True)
        sys.exit(1)  # nothing more on a device that may be hung
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode or not line:
        print(json.dumps({"args": args, "error": r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
        sys.exit(1)  # a failed child ends the sweep
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds per process")
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="c5,c4,c3")
    ap.add_argument("--parent-tree", default="", help="a checkout of the parent commit, built: the ordinary steps' A/B")
    ap.add_argument("--only", default="", help="one shape's name (a child process)")
    ap.add_argument("--steps-in", default="", help="with --only: the ordinary steps alone, in this tree")
    a = ap.parse_args()
    if a.steps < 64 or a.reps < 3:
        ap.error("at least 64 steps and 3 alternating repetitions")
    if a.only:
        C, B, P = SHAPES[a.only]
        if a.steps_in:
            child_steps(a.steps_in, C, B, P, a.steps, a.warmup)
        else:
            child(C, B, P, a.steps, a.warmup, a.reps)
        return
    out = {"points": []}
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    for name in a.shapes.split(","):
        pt = {"shape": name, **run_child(["--only", name] + common, a.limit)}
        if a.parent_tree:
            trees = {"this": os.path.abspath(os.path.join(HERE, "..")), "parent": os.path.abspath(a.parent_tree)}
            ab = {n: {"plain_step": [], "stream_step": []} for n in trees}
            for _ in range(a.reps):  # the trees alternate
                for n, tree in trees.items():
                    r = run_child(["--only", name, "--steps-in", tree] + common, a.limit)
                    for k in ab[n]:
                        ab[n][k].append(r[k])
            pt["steps_ab"] = {n: {k: {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}
                                  for k, v in d.items()} for n, d in ab.items()}
        out["points"].append(pt)
        print(json.dumps(pt), flush=True)
        if a.out:  # after every point: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

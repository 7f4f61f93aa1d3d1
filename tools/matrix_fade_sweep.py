"""The matrix convolver's fade step (a live filter update, neo.MatrixConvolver.update_filter) against
the form a user has without it, at B = 512: GPU time per block, between two stream events over
`--steps` back-to-back steps after a warm-up, of

  (a) step        the ordinary block step,
  (b) fade_step   the fade step: an update over `--steps` blocks, then that many single-block calls
                  (three launches each: windows, both banks against the same delay-line rows, two
                  inverse transforms and the mix),
  (c) two_handles what stands in for it without the feature: two MatrixConvolver handles (filters A
                  and B) stepping the same block, and torch.lerp of their outputs with the block's
                  gains on the device,
  (d) update      the update_filter call itself with a device tensor (fade_blocks = 1, the fade's
                  one block run untimed after it): host wall time of the call and GPU time between
                  two events around it,

for dense 2 x 2 and 32 x 32 at P = 32 and dense 8 x 32 at P = 128. Every variant is timed `--reps`
times, the variants alternating, so the spread of each is that of the same A/B on the same box. One
process per configuration, each under its own time limit.
--parent-tree DIR (a checkout of the parent commit with its library built): (a) once more there,
in processes that alternate with this tree's, `--reps` times each: the step path's same-run A/B.
Run once on an MI355X:  python tools/matrix_fade_sweep.py --out profiles/matrix_fade_sweep.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B = 512
CONFIGS = [(2, 2, 32), (32, 32, 32), (8, 32, 128)]  # I, O, P


def setup(tree, I, O, P):
    import torch

    sys.path.insert(0, os.path.join(tree, "neo-dsp_amd"))
    import neo

    routes = [(o, i) for o in range(O) for i in range(I)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    mk = lambda: torch.view_as_complex(torch.rand((len(routes), P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / (P * I))
    pa, pb = mk(), mk()
    nblk = 8
    x = torch.rand((I, B * nblk), device="cuda", generator=gen) * 2 - 1
    y = torch.empty((O, B * nblk), device="cuda")
    return torch, neo, routes, pa, pb, nblk, x, y


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


def child_step(tree, I, O, P, steps, warm):
    """(a) alone, in the tree given: one figure"""
    torch, neo, routes, pa, _, nblk, x, y = setup(tree, I, O, P)
    s = torch.cuda.current_stream().cuda_stream
    conv = neo.MatrixConvolver(I, O, B, P)
    conv.filter(pa, routes)

    def step(t):
        o = 4 * (t % nblk) * B
        conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], 1, s)

    for t in range(warm):
        step(t)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"us": timed(torch, step, steps)}), flush=True)


def child(I, O, P, steps, warm, reps):
    torch, neo, routes, pa, pb, nblk, x, y = setup(os.path.join(HERE, ".."), I, O, P)
    s = torch.cuda.current_stream().cuda_stream
    banks = [pa, pb]

    def handle(parts):
        conv = neo.MatrixConvolver(I, O, B, P)
        conv.filter(parts, routes)
        return conv

    plain, fading, ha, hb, upd = handle(pa), handle(pa), handle(pa), handle(pb), handle(pa)
    ya, yb = torch.empty((O, B), device="cuda"), torch.empty((O, B), device="cuda")
    g = torch.from_numpy(neo.matrix_fade_gains(B, 1, "linear")).cuda()
    flip = {"n": 0}

    def step_of(conv):
        def step(t):
            o = 4 * (t % nblk) * B
            conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], 1, s)
        return step

    def arm():  # a fade over exactly the timed steps: the handle is back to passes after them
        flip["n"] += 1
        fading.update_filter(banks[flip["n"] % 2], fade_blocks=steps)

    def two(t):
        o = 4 * (t % nblk) * B
        ha.process_device(x.data_ptr() + o, x.shape[1], ya.data_ptr(), B, 1, s)
        hb.process_device(x.data_ptr() + o, x.shape[1], yb.data_ptr(), B, 1, s)
        torch.lerp(ya, yb, g, out=y[:, (t % nblk) * B:(t % nblk + 1) * B])

    def update_times(n):
        host, gpu = [], []
        for k in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            upd.update_filter(banks[(k + 1) % 2], fade_blocks=1)
            host.append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            gpu.append(e0.elapsed_time(e1) * 1e3)
            step_of(upd)(k)  # the fade's one block: the next update is allowed
        return float(np.median(host)), float(np.median(gpu))

    variants = {"step": (step_of(plain), None), "fade_step": (step_of(fading), arm), "two_handles": (two, None)}
    for step, before in variants.values():
        if before:
            before()
        for t in range(max(warm, steps) if before else warm):  # the warm-up fade runs to its end
            step(t)
    update_times(4)
    torch.cuda.synchronize()
    us = {n: [] for n in variants}
    up = []
    for _ in range(reps):  # the variants alternate
        for n, (step, before) in variants.items():
            us[n].append(timed(torch, step, steps, before))
        up.append(update_times(16))
    assert fading.fade_info()["remaining_blocks"] == 0
    info = plain.info()
    res = {"inputs": I, "outputs": O, "block": B, "partitions": P, "routes": len(routes), "steps": steps, "warmup": warm,
           "reps": reps, "step_plan": {k: info[k] for k in ("out_tile", "splits", "fused", "tiles")},
           "bank_bytes": fading.fade_info()["bank_bytes"], "variants": {}}
    for n, v in us.items():
        res["variants"][n] = {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}
    res["variants"]["update"] = {"host_us": round(float(np.median([h for h, _ in up])), 2),
                                 "host_us_min_max": [round(min(h for h, _ in up), 2), round(max(h for h, _ in up), 2)],
                                 "gpu_us": round(float(np.median([q for _, q in up])), 2),
                                 "gpu_us_min_max": [round(min(q for _, q in up), 2), round(max(q for _, q in up), 2)]}
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
    ap.add_argument("--parent-tree", default="", help="a checkout of the parent commit, built: the step's A/B")
    ap.add_argument("--only", default="", help="I,O,P of one configuration (a child process)")
    ap.add_argument("--step-in", default="", help="with --only: the ordinary step alone, in this tree")
    a = ap.parse_args()
    if a.steps < 64 or a.reps < 3:
        ap.error("at least 64 steps and 3 alternating repetitions")
    if a.only:
        I, O, P = (int(v) for v in a.only.split(","))
        if a.step_in:
            child_step(a.step_in, I, O, P, a.steps, a.warmup)
        else:
            child(I, O, P, a.steps, a.warmup, a.reps)
        return
    out = {"block": B, "points": []}
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    for I, O, P in CONFIGS:
        pt = run_child(["--only", f"{I},{O},{P}"] + common, a.limit)
        if a.parent_tree:
            trees = {"this": os.path.abspath(os.path.join(HERE, "..")), "parent": os.path.abspath(a.parent_tree)}
            ab = {n: [] for n in trees}
            for _ in range(a.reps):  # the trees alternate
                for n, tree in trees.items():
                    ab[n].append(run_child(["--only", f"{I},{O},{P}", "--step-in", tree] + common, a.limit)["us"])
            pt["step_ab"] = {n: {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}
                             for n, v in ab.items()}
        out["points"].append(pt)
        print(json.dumps(pt), flush=True)
        if a.out:  # after every point: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

"""The sparse convolvers' fade step (a live filter update, neo.SparseUpolsConvolver.update_filter)
beside the two sparse steps it stands in for, at 256 x 512 x 938. GPU time per block, between two
stream events over `--steps` back-to-back single-block calls after a warm-up. Points (mask A -> B, at
tile densities): random tiles 0.25 -> 0.10 and 0.10 -> 0.25, nested; 0.10 -> 0.10, independent; the
decaying mask 0.05 -> 0.10. Per point, all handles alive in one process:

  (a) fade_step   an update A -> B over `--steps` blocks, then that many calls (two launches each);
                  the fade back B -> A runs untimed between the repetitions,
  (b) step_a, step_b   the sparse step of a handle with A alone and of one with B alone: their sum is
                  what two warmed-up handles would cost per block (the bar: the fade step stays below it),
  (c) update      the update_filter call itself with device tensors (fade_blocks = 1): host wall time
                  and GPU time between two events around it,
  (d) model       neo.sparse_fade_plan's bytes at 8 TB/s, and the ratio the bytes predict,
                  (t_A + t_B + t_AuB) / (2 t_A + 2 t_B) in kept tiles.

Every variant is timed `--reps` times, the variants alternating. One process per point, each under
its own time limit. --parent-tree DIR (a checkout of the parent commit with its library built): the
sparse step on A and on B once more there, in processes that alternate with this tree's.
Run once on an MI355X:  python tools/sparse_fade_sweep.py --out profiles/sparse_fade_sweep.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
C, B, P = 256, 512, 938
PEAK = 8.0e12  # bytes / s
POINTS = {"nested_0.25_to_0.10": ("nested", 0.25, 0.10), "nested_0.10_to_0.25": ("nested", 0.10, 0.25),
          "random_0.10_to_0.10": ("independent", 0.10, 0.10), "decaying_0.05_to_0.10": ("decaying", 0.05, 0.10)}


def expand_tiles(torch, keep):
    """[C][P][NT] kept tiles -> [C][P][B+1] columns (columns 0 and B lie in tile 0)"""
    cols = keep.repeat_interleave(16, dim=2)
    return torch.cat([cols, keep[:, :, :1]], dim=2).to(torch.uint8).contiguous()


def decaying(torch, d):
    """column k of partition p kept iff k <= floor(B 0.5^(p / tau)); tau by bisection for tile density d"""
    p = np.arange(P)

    def tiles(tau):
        return np.minimum(B // 16, np.floor(B * 0.5 ** (p / tau)).astype(np.int64) // 16 + 1)

    lo, hi = 1e-3, 1e7
    for _ in range(80):
        mid = (lo * hi) ** 0.5
        lo, hi = (mid, hi) if tiles(mid).mean() < d * (B // 16) else (lo, mid)
    lim = torch.from_numpy(np.floor(B * 0.5 ** (p / hi)).astype(np.int64)).cuda()
    k = torch.arange(B + 1, device="cuda")
    return (k[None, :] <= lim[:, None])[None].expand(C, P, B + 1).to(torch.uint8).contiguous()


def setup(tree, point):
    import torch

    sys.path.insert(0, os.path.join(tree, "neo-dsp_amd"))
    import neo

    kind, da, db = POINTS[point]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    mk = lambda: torch.view_as_complex(torch.rand((C, P, B + 1, 2), device="cuda", generator=gen) * 2 - 1) * (1.0 / P)
    parts = [mk(), mk()]
    u = torch.rand((C, P, B // 16), device="cuda", generator=gen)
    if kind == "nested":
        masks = [expand_tiles(torch, u < da), expand_tiles(torch, u < db)]
    elif kind == "independent":
        v = torch.rand((C, P, B // 16), device="cuda", generator=gen)
        masks = [expand_tiles(torch, u < da), expand_tiles(torch, v < db)]
    else:
        masks = [decaying(torch, da), decaying(torch, db)]
    nblk = 8
    x = torch.rand((C, B * nblk), device="cuda", generator=gen) * 2 - 1
    y = torch.empty((C, B * nblk), device="cuda")
    return torch, neo, parts, masks, nblk, x, y


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


def stepper(conv, nblk, x, y, s):
    def step(t):
        o = 4 * (t % nblk) * B
        conv.process_device(x.data_ptr() + o, x.shape[1], y.data_ptr() + o, y.shape[1], s)
    return step


def handle(neo, parts, mask):
    conv = neo.SparseUpolsConvolver(C, B, P)
    conv.filter(parts, mask)
    return conv


def child_steps(tree, point, steps, warm):
    """(b) alone, in the tree given"""
    torch, neo, parts, masks, nblk, x, y = setup(tree, point)
    s = torch.cuda.current_stream().cuda_stream
    res = {}
    for name, i in (("step_a", 0), ("step_b", 1)):
        conv = handle(neo, parts[i], masks[i])
        step = stepper(conv, nblk, x, y, s)
        for t in range(warm):
            step(t)
        torch.cuda.synchronize()
        res[name] = timed(torch, step, steps)
        conv.close()
    print("RESULT " + json.dumps(res), flush=True)


def child(point, steps, warm, reps):
    torch, neo, parts, masks, nblk, x, y = setup(os.path.join(HERE, ".."), point)
    s = torch.cuda.current_stream().cuda_stream
    plan = neo.sparse_fade_plan(masks[0].cpu().numpy(), masks[1].cpu().numpy(), B)
    ha, hb, fading, upd = (handle(neo, parts[i], masks[i]) for i in (0, 1, 0, 0))
    assert plan["splits"] == fading.splits
    fstep = stepper(fading, nblk, x, y, s)

    state = {"on_b": False}

    def arm():  # back to A (a fade of one block, untimed), then A -> B over exactly the timed steps
        if state["on_b"]:
            fading.update_filter(parts[0], masks[0], fade_blocks=1, stream=s)
            fstep(0)
        fading.update_filter(parts[1], masks[1], fade_blocks=steps, stream=s)
        state["on_b"] = True

    def update_times(n):
        host, gpu = [], []
        one = stepper(upd, nblk, x, y, s)
        for k in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            upd.update_filter(parts[(k + 1) % 2], masks[(k + 1) % 2], fade_blocks=1, stream=s)
            host.append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            gpu.append(e0.elapsed_time(e1) * 1e3)
            one(k)  # the fade's one block: the next update is allowed
        return float(np.median(host)), float(np.median(gpu))

    variants = {"fade_step": (fstep, arm), "step_a": (stepper(ha, nblk, x, y, s), None), "step_b": (stepper(hb, nblk, x, y, s), None)}
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
        up.append(update_times(3))
    assert fading.fade_info()["remaining_blocks"] == 0
    tiles = C * P * (B // 16)
    res = {"channels": C, "block": B, "partitions": P, "steps": steps, "warmup": warm, "reps": reps, "splits": fading.splits,
           "tile_density": {k: round(plan["tiles_" + k] / tiles, 4) for k in ("a", "b", "union")}, "plan": plan,
           "spare_bank_bytes": fading.fade_info()["bank_bytes"], "variants": {}}

    def stat(v, key="us"):
        return {key: round(float(np.median(v)), 2), key + "_min_max": [round(min(v), 2), round(max(v), 2)]}

    for n, v in us.items():
        res["variants"][n] = stat(v)
    res["variants"]["update"] = {**stat([h for h, _ in up], "host_us"), **stat([q for _, q in up], "gpu_us")}
    both = res["variants"]["step_a"]["us"] + res["variants"]["step_b"]["us"]
    res["two_steps_us"] = round(both, 2)
    res["fade_over_two_steps"] = round(res["variants"]["fade_step"]["us"] / both, 3)
    res["bar_met"] = bool(max(us["fade_step"]) < min(us["step_a"]) + min(us["step_b"]))
    res["model_ratio"] = round((plan["tiles_a"] + plan["tiles_b"] + plan["tiles_union"]) /
                               (2.0 * plan["tiles_a"] + 2.0 * plan["tiles_b"]), 3)
    res["model_us_at_8TBs"] = round(plan["step_bytes"] / PEAK * 1e6, 2)
    res["fraction_of_peak"] = round(plan["step_bytes"] / (res["variants"]["fade_step"]["us"] * 1e-6) / PEAK, 4)
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
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--parent-tree", default="", help="a checkout of the parent commit, built: the sparse step's A/B")
    ap.add_argument("--only", default="", help="one point's name (a child process)")
    ap.add_argument("--steps-in", default="", help="with --only: the sparse steps alone, in this tree")
    a = ap.parse_args()
    if a.steps < 64 or a.reps < 3:
        ap.error("at least 64 steps and 3 alternating repetitions")
    if a.only:
        if a.steps_in:
            child_steps(a.steps_in, a.only, a.steps, a.warmup)
        else:
            child(a.only, a.steps, a.warmup, a.reps)
        return
    out = {"shape": {"channels": C, "block": B, "partitions": P}, "points": []}
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    for name in a.points.split(","):
        pt = {"point": name, **run_child(["--only", name] + common, a.limit)}
        if a.parent_tree:
            trees = {"this": os.path.abspath(os.path.join(HERE, "..")), "parent": os.path.abspath(a.parent_tree)}
            ab = {n: {"step_a": [], "step_b": []} for n in trees}
            for _ in range(a.reps):  # the trees alternate
                for n, tree in trees.items():
                    r = run_child(["--only", name, "--steps-in", tree] + common, a.limit)
                    for k in ab[n]:
                        ab[n][k].append(r[k])
            pt["steps_ab"] = {n: {k: {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}
                                  for k, v in d.items()} for n, d in ab.items()}
            pt["steps_ab_overlap"] = {k: bool(min(ab["this"][k]) <= max(ab["parent"][k]) and min(ab["parent"][k]) <= max(ab["this"][k]))
                                      for k in ("step_a", "step_b")}
        out["points"].append(pt)
        print(json.dumps(pt), flush=True)
        if a.out:  # after every point: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

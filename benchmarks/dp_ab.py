#!/usr/bin/env python3
"""Differential-privacy A/B: per-op cost, round cost and accuracy.

Part `ops`: device-event time of the update extraction and the privacy
kernels on flat fp32 vectors of P = 428350 (FEMNIST CNN, P % 4 == 2),
272474 (ResNet-20) and 25.6 M coordinates. Algorithmic bytes: the
extraction reads two vectors and writes one (12 B per coordinate), the
stand-alone sum of squares reads one (4 B), dp_privatize_ reads and
writes one (8 B). GB/s = bytes / time; the two small vectors fit in the
caches, so only the 25.6 M row is an HBM figure.

Part `rounds`: FEMNIST ms/round of the bench.py configuration with the
feature off, clip only, local noise and central noise — four engines in
ONE process, rounds interleaved, median and min over --rounds rounds.

Part `accuracy`: sponsor accuracy after --acc-rounds rounds over a grid
of noise multipliers, local and central.

Part `bench`: `bench.py --gpus 1` in each tree of --trees (this one and,
for instance, a checkout of the parent commit), alternating, --repeats
times each; reports every ms/round so that the run-to-run spread is
visible next to the difference.

Each GPU step runs in a fresh child process under its own `timeout`,
one at a time; the first failure stops the script (no retries).

    python benchmarks/dp_ab.py [--part ops,rounds,accuracy] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = (428350, 272474, 25_600_000)
Z_GRID = (0.0, 0.001, 0.01, 0.1)
FEMNIST = dict(model="femnist_cnn", n_class=62, partition="dirichlet",
               dirichlet_alpha=0.3, learning_rate=0.01)
# model-space bound of the round/accuracy parts; whether it binds shows
# in the applied clip coefficients the `rounds` part reports
CLIP = 1.0
ACC_CLIP = 0.1
VARIANTS = {
    "off": dict(),
    "clip_only": dict(dp_clip=CLIP),
    "local_noise": dict(dp_clip=CLIP, dp_noise_multiplier=0.01),
    "central_noise": dict(dp_clip=CLIP, dp_noise_multiplier=0.01,
                          dp_mode="central"),
}


def time_op(fn, iters: int) -> float:
    """Median device-event milliseconds of fn() over `iters` calls."""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def run_ops(args, P: int) -> list:
    import torch
    from bflc_amd.ops import functional as O
    assert torch.cuda.is_available(), "dp_ab ops needs a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(0)
    g = torch.randn(P, generator=gen).to(dev)
    w = g + 0.01 * torch.randn(P, generator=gen).to(dev)
    out = torch.empty_like(g)
    off = torch.empty(P + 1, device=dev)[1:]      # 4 bytes off: dword path
    coef = torch.empty(2, device=dev)
    half = torch.full((1,), 0.5, device=dev)
    part = torch.empty(O.sumsq_partials(P, dev), device=dev)
    lr = 0.01

    def two_pass():
        O.delta_extract_(out, g, w, lr)
        O.grad_clip_coef_(out, 1.0, coef)

    def fused():
        O.delta_extract_sumsq_(out, g, w, lr, part)
        O.grad_clip_final_(part, 1.0, coef)

    # (name, bytes per coordinate, fn)
    ops = [
        ("delta_extract_", 12, lambda: O.delta_extract_(out, g, w, lr)),
        ("delta_extract_ + grad_clip_coef_", 16, two_pass),
        ("delta_extract_sumsq_ + grad_clip_final_", 12, fused),
        ("dp_privatize_ sigma=0 (clip)", 8,
         lambda: O.dp_privatize_(out, half, 0.0, 1, 0, 0)),
        ("dp_privatize_ noise, float4", 8,
         lambda: O.dp_privatize_(out, half, 1.0, 1, 0, 0)),
        ("dp_privatize_ noise, dword", 8,
         lambda: O.dp_privatize_(off, half, 1.0, 1, 0, 0)),
    ]
    rows = []
    for name, bpc, fn in ops:
        ms = time_op(fn, args.iters)
        rows.append({"P": P, "op": name, "ms": round(ms, 4),
                     "GBps": round(P * bpc / (ms * 1e-3) / 1e9, 1),
                     "Gcoord_s": round(P / (ms * 1e-3) / 1e9, 2)})
    return rows


def _engine(args, **kw):
    import torch
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    cfg = FLConfig.for_world(8, samples_per_client=args.samples,
                             batch_size=args.batch,
                             eval_samples=min(4096, 2 * args.samples),
                             seed=args.seed, **FEMNIST, **kw)
    shards, test = make_federated(cfg)
    return FLEngine(cfg, Transport(device=torch.device(args.device)),
                    shards, test)


def run_rounds(args) -> list:
    import gc
    engines = {name: _engine(args, **kw) for name, kw in VARIANTS.items()}
    for eng in engines.values():
        eng.run(3)                                  # capture + warm up
    wall = {name: [] for name in engines}
    gc.collect()
    gc.disable()
    for _ in range(args.rounds):                    # interleaved
        for name, eng in engines.items():
            wall[name].append(eng.run_round().wall_s * 1e3)
    gc.enable()
    rows = []
    for name, ts in wall.items():
        p = engines[name].last_privacy
        coefs = sorted(p["clip_coef"].values()) if p else []
        rows.append({"variant": name, "rounds": len(ts),
                     "median_ms": round(statistics.median(ts), 3),
                     "min_ms": round(min(ts), 3),
                     "max_ms": round(max(ts), 3),
                     "clip_coef_last_round":
                         [round(c, 3) for c in coefs]})
    return rows


def run_accuracy(args, mode: str, z: float) -> dict:
    kw = dict(dp_clip=ACC_CLIP, dp_noise_multiplier=z, dp_mode=mode)
    if mode == "off":
        kw = {}
    eng = _engine(args, **kw)
    eng.run(args.acc_rounds)
    p = eng.last_privacy
    coefs = sorted(p["clip_coef"].values()) if p else []
    return {"mode": mode, "z": z, "rounds": args.acc_rounds,
            "acc": round(float(eng.evaluate_global()), 4),
            "epsilon": p["epsilon"] if p else None,
            "clip_coef_last_round": [round(c, 3) for c in coefs]}


def child(args, what: str) -> list:
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable,
           os.path.abspath(__file__), "--run", what]
    for k in ("iters", "rounds", "acc_rounds", "seed", "device", "samples",
              "batch"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(res.stdout)
    sys.stdout.flush()
    if res.returncode != 0:
        raise SystemExit(f"dp_ab: {what} exited with {res.returncode}; "
                         "stopping")
    return [json.loads(line[len("DP_AB "):])
            for line in res.stdout.splitlines()
            if line.startswith("DP_AB ")]


def bench_tree(args, tree: str) -> float:
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable,
           "bench.py", "--gpus", "1", "--steps", str(args.bench_steps),
           "--warmup", str(args.bench_warmup)]
    res = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, text=True)
    if res.returncode != 0:
        raise SystemExit(f"dp_ab: bench.py in {tree} exited with "
                         f"{res.returncode}; stopping")
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    return float(json.loads(line)["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ops,rounds,accuracy")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--acc-rounds", type=int, default=30)
    ap.add_argument("--samples", type=int, default=3072)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--trees", default=REPO,
                    help="bench: comma-separated checkouts to compare")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed for each child process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "r13_dp_ab.md"))
    ap.add_argument("--run", default=None,
                    help="(child) ops:P | rounds | accuracy:MODE:Z")
    args = ap.parse_args()
    if args.run is not None:
        kind, _, rest = args.run.partition(":")
        if kind == "ops":
            rows = run_ops(args, int(rest))
        elif kind == "rounds":
            rows = run_rounds(args)
        else:
            mode, z = rest.split(":")
            rows = [run_accuracy(args, mode, float(z))]
        for row in rows:
            print("DP_AB " + json.dumps(row), flush=True)
        return

    parts = args.part.split(",")
    md = ["# Round 13: differential privacy A/B (benchmarks/dp_ab.py)", ""]
    if "ops" in parts:
        rows = []
        for P in args.sizes.split(","):
            rows += child(args, f"ops:{P}")
        md += ["## Per-op time (median of device events)", "",
               "| P | op | ms | GB/s (algorithmic) | G coord/s |",
               "|---|---|---|---|---|"]
        md += [f"| {r['P']} | {r['op']} | {r['ms']:.4f} | {r['GBps']:.0f} | "
               f"{r['Gcoord_s']:.2f} |" for r in rows]
        md.append("")
    if "rounds" in parts:
        rows = child(args, "rounds")
        md += [f"## FEMNIST ms/round, 8 clients, {args.samples} samples, "
               f"batch {args.batch}; interleaved in one process", "",
               "| variant | rounds | median ms | min ms | max ms | clip "
               "coefficients, last round |", "|---|---|---|---|---|---|"]
        md += [f"| {r['variant']} | {r['rounds']} | {r['median_ms']:.2f} | "
               f"{r['min_ms']:.2f} | {r['max_ms']:.2f} | "
               f"{r['clip_coef_last_round']} |" for r in rows]
        md.append("")
    if "accuracy" in parts:
        rows = child(args, "accuracy:off:0")
        for mode in ("local", "central"):
            for z in Z_GRID:
                rows += child(args, f"accuracy:{mode}:{z}")
        md += [f"## Sponsor accuracy after {args.acc_rounds} rounds, "
               f"dp_clip = {ACC_CLIP}", "",
               "| mode | z | accuracy | epsilon (delta 1e-5) | clip "
               "coefficients, last round |", "|---|---|---|---|---|"]
        md += [f"| {r['mode']} | {r['z']} | {r['acc']:.4f} | "
               + ("-" if r["epsilon"] is None else f"{r['epsilon']:.3g}")
               + f" | {r['clip_coef_last_round']} |" for r in rows]
        md.append("")
    if "bench" in parts:
        trees = args.trees.split(",")
        vals = {t: [] for t in trees}
        for _ in range(args.repeats):               # alternating
            for t in trees:
                vals[t].append(bench_tree(args, t))
                print(f"DP_AB bench {t}: {vals[t][-1]:.3f} ms/round",
                      flush=True)
        md += [f"## bench.py --gpus 1 --steps {args.bench_steps} --warmup "
               f"{args.bench_warmup}, alternating, ms/round", "",
               "| tree | runs | median |", "|---|---|---|"]
        md += [f"| {os.path.relpath(t, REPO)} | "
               f"{', '.join(f'{v:.2f}' for v in vs)} | "
               f"{statistics.median(vs):.2f} |" for t, vs in vals.items()]
        md.append("")
    text = "\n".join(md)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

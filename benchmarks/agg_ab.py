#!/usr/bin/env python3
"""Robust-aggregation A/B: per-op timing and an aggregator x attack grid.

Part `ops`: device-event time of order_stat_mean (t = 1 and the median),
delta_gram, masked_wmean and weighted_fedavg on ONE [K, P] fp32 buffer
per shape, K in {3, 10, 32}, P of the FEMNIST CNN (428350, P % 4 == 2),
ResNet-20 and ResNet-50. Every op reads the same K * P * 4 bytes once,
so time / time(weighted_fedavg) is the yardstick; GB/s is K*P*4 / time.
(weighted_fedavg mis-addresses rows at P % 4 != 0 — its time there is
still the time of reading the same bytes.)

Part `grid`: final sponsor accuracy of aggregator x attack on the MLP
and the FEMNIST CNN, 8 clients / committee 2 / quota 6 with
aggregate_count = needed_update_count (the committee passes everything,
each rule stands alone), 2 attackers.

Each GPU step runs in a fresh child process under its own `timeout`,
one at a time; the first failure stops the script (no retries).

    python benchmarks/agg_ab.py [--part ops,grid] [--device cuda]
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (3, 10, 32)
MODEL_P = {"femnist_cnn": dict(model="femnist_cnn", n_class=62),
           "resnet20": dict(model="resnet20", n_class=10),
           "resnet50": dict(model="resnet50", n_class=1000)}

GRID_MODELS = {
    "mlp": dict(model="mlp", n_features=32, n_class=8,
                samples_per_client=256, batch_size=128, eval_samples=1024,
                learning_rate=0.05),
    "femnist": dict(model="femnist_cnn", n_class=62,
                    samples_per_client=1024, batch_size=256,
                    eval_samples=2048, learning_rate=0.05),
}
ATTACKS = {"none": dict(byzantine_clients=0),
           "label_flip": dict(byzantine_clients=2),
           "scale-4": dict(byzantine_clients=2, byzantine_attack="scale",
                           byzantine_scale=-4.0)}
AGGS = ("fedavg", "trimmed_mean", "median", "multi_krum")


def model_params(key: str) -> int:
    import torch
    from bflc_amd.config import FLConfig
    from bflc_amd.models import build_model
    cfg = FLConfig(**MODEL_P[key])
    return int(build_model(cfg, torch.device("cpu")).get_flat().numel())


def time_op(fn, iters: int) -> float:
    """Median device-event milliseconds of fn() over `iters` calls."""
    import torch
    for _ in range(3):
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
    ts.sort()
    return ts[len(ts) // 2]


def run_ops(args, key: str) -> list:
    import torch
    from bflc_amd.ops import functional as O
    assert torch.cuda.is_available(), "agg_ab ops needs a GPU"
    P = model_params(key)
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for K in KS:
        d = torch.randn(K, P, generator=gen).to(dev)
        w = torch.arange(1, K + 1, dtype=torch.float32, device=dev)
        ops = {
            "weighted_fedavg": lambda: O.weighted_fedavg(d, w),
            "masked_wmean": lambda: O.masked_wmean(d, w),
            "order_stat_mean_t1": lambda: O.order_stat_mean(d, 1),
            "order_stat_mean_median":
                lambda: O.order_stat_mean(d, (K - 1) // 2),
            "delta_gram": lambda: O.delta_gram(d),
        }
        ms = {name: time_op(fn, args.iters) for name, fn in ops.items()}
        base = ms["weighted_fedavg"]
        for name, v in ms.items():
            rows.append({"model": key, "P": P, "K": K, "op": name,
                         "ms": round(v, 4), "ratio": round(v / base, 3),
                         "GBps": round(K * P * 4 / (v * 1e-3) / 1e9, 1)})
        del d
    return rows


def run_grid(args, model_key: str, agg: str, attack: str) -> dict:
    import torch
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    dev = torch.device(args.device)
    cfg = FLConfig(client_num=8, comm_count=2, needed_update_count=6,
                   aggregate_count=6, aggregator=agg, seed=args.seed,
                   **GRID_MODELS[model_key], **ATTACKS[attack])
    shards, test = make_federated(cfg)
    t = Transport(device=dev)
    eng = FLEngine(cfg, t, shards, test)
    attackers = {f"node_{i}" for i in range(8) if shards[i].byzantine}
    kept_bad = 0
    for _ in range(args.rounds):
        eng.run_round()
        kept_bad += len(attackers &
                        set(eng.last_aggregation.get("kept", [])))
    acc = float(eng.evaluate_global())
    t.close()
    return {"model": model_key, "aggregator": agg, "attack": attack,
            "seed": args.seed, "rounds": args.rounds, "device": args.device,
            "acc": round(acc, 4), "krum_kept_attackers": kept_bad}


def child(args, what: str) -> list:
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable,
           os.path.abspath(__file__), "--run", what, "--iters",
           str(args.iters), "--rounds", str(args.rounds), "--seed",
           str(args.seed), "--device", args.device]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(res.stdout)
    sys.stdout.flush()
    if res.returncode != 0:
        raise SystemExit(f"agg_ab: {what} exited with {res.returncode}; "
                         "stopping")
    return [json.loads(line[len("AGG_AB "):])
            for line in res.stdout.splitlines()
            if line.startswith("AGG_AB ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ops,grid")
    ap.add_argument("--models", default="femnist_cnn,resnet20,resnet50")
    ap.add_argument("--grid-models", default="mlp,femnist")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--step-timeout", type=int, default=180,
                    help="seconds allowed for each child process")
    ap.add_argument("--run", default=None,
                    help="(child) ops:MODEL or grid:MODEL:AGG:ATTACK")
    args = ap.parse_args()
    if args.run is not None:
        kind, rest = args.run.split(":", 1)
        if kind == "ops":
            for row in run_ops(args, rest):
                print("AGG_AB " + json.dumps(row), flush=True)
        else:
            m, agg, attack = rest.split(":")
            print("AGG_AB " + json.dumps(run_grid(args, m, agg, attack)),
                  flush=True)
        return
    parts = args.part.split(",")
    if "ops" in parts:
        rows = []
        for key in args.models.split(","):
            rows += child(args, f"ops:{key}")
        print("| model | P | K | op | ms | x fedavg | GB/s |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['model']} | {r['P']} | {r['K']} | {r['op']} | "
                  f"{r['ms']:.4f} | {r['ratio']:.2f} | {r['GBps']:.0f} |")
    if "grid" in parts:
        rows = []
        for m in args.grid_models.split(","):
            for attack in ATTACKS:
                for agg in AGGS:
                    rows += child(args, f"grid:{m}:{agg}:{attack}")
        print("| model | attack | aggregator | acc | attackers kept by "
              "Krum |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['model']} | {r['attack']} | {r['aggregator']} | "
                  f"{r['acc']:.4f} | {r['krum_kept_attackers']} |")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Local-optimizer A/B under the committee protocol.

Runs the protocol configs (FEMNIST CNN, ResNet-20 with BatchNorm,
ResNet-20 with GroupNorm; 8 clients / committee 4, Dirichlet(0.3)
shards, the bench.py shapes) for a fixed number of rounds under a small
grid of local steps, same seed and rounds for every row:

  legacy           the default sgd_master_ step
  mom              momentum 0.9
  mom+cos          + cosine decay of the local lr over the run
  mom+cos+clip     + global-norm clip
  mom+cos+clip+prox  + FedProx proximal term

and prints, per row, the sponsor test accuracy (best over the periodic
evaluations, and final) and ms/round (mean run_round wall time after
the warm-up rounds; evaluation is outside it).

Each row runs in a fresh child process under its own `timeout`, one at
a time; the first failure stops the script (no retries).

    python benchmarks/optim_ab.py [--rounds 300] [--models femnist,r20bn,r20gn]
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {
    "femnist": dict(model="femnist_cnn", n_class=62, samples_per_client=3072,
                    batch_size=1024),
    "r20bn": dict(model="resnet20", n_class=10, samples_per_client=2048,
                  batch_size=512, norm_groups=0),
    "r20gn": dict(model="resnet20", n_class=10, samples_per_client=2048,
                  batch_size=512, norm_groups=8),
}


def grid(args):
    mom = dict(momentum=args.momentum)
    cos = dict(mom, lr_schedule="cosine", lr_total_rounds=args.rounds)
    clip = dict(cos, clip_norm=args.clip)
    return [("legacy", {}), ("mom", mom), ("mom+cos", cos),
            ("mom+cos+clip", clip),
            ("mom+cos+clip+prox", dict(clip, prox_mu=args.mu))]


def run_row(args, model_key: str, row: str) -> dict:
    import torch
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine

    assert torch.cuda.is_available(), "optim_ab needs a GPU"
    md = MODELS[model_key]
    cfg = FLConfig.for_world(
        8, partition="dirichlet", dirichlet_alpha=0.3,
        eval_samples=min(4096, 2 * md["samples_per_client"]),
        learning_rate=args.lr, max_epoch=args.rounds + 10,
        **md, **dict(grid(args))[row])
    t = Transport()
    shards, test = make_federated(cfg)
    eng = FLEngine(cfg, t, shards, test)
    walls, accs = [], []
    for r in range(args.rounds):
        st = eng.run_round()
        if r >= args.warmup:
            walls.append(st.wall_s)
        if (r + 1) % args.eval_every == 0 or r + 1 == args.rounds:
            accs.append(float(eng.evaluate_global()))
    finite = bool(torch.isfinite(eng.global_flat).all())
    t.close()
    return {"model": model_key, "row": row,
            "local_optimizer": eng.local_optimizer,
            "best_acc": round(max(accs), 4), "final_acc": round(accs[-1], 4),
            "ms_per_round": round(1e3 * sum(walls) / max(len(walls), 1), 3),
            "finite": finite, "rounds": args.rounds, "lr": args.lr,
            "chance": round(1.0 / md["n_class"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval-every", type=int, default=25)
    ap.add_argument("--models", default="femnist,r20bn,r20gn")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--clip", type=float, default=2.0)
    ap.add_argument("--mu", type=float, default=0.01)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed for each row's child process")
    ap.add_argument("--run", default=None,
                    help="(child) run one row: MODEL:ROW")
    args = ap.parse_args()
    if args.run is not None:
        model_key, row = args.run.split(":", 1)
        print("OPTIM_AB " + json.dumps(run_row(args, model_key, row)),
              flush=True)
        return
    passthrough = ["--rounds", args.rounds, "--warmup", args.warmup,
                   "--eval-every", args.eval_every, "--lr", args.lr,
                   "--momentum", args.momentum, "--clip", args.clip,
                   "--mu", args.mu]
    rows = []
    for model_key in args.models.split(","):
        for row, _ in grid(args):
            cmd = ["timeout", "-k", "10", str(args.step_timeout),
                   sys.executable, os.path.abspath(__file__), "--run",
                   f"{model_key}:{row}"] + [str(a) for a in passthrough]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"optim_ab: {model_key}:{row} exited with "
                                 f"{res.returncode}; stopping")
            for line in res.stdout.splitlines():
                if line.startswith("OPTIM_AB "):
                    rows.append(json.loads(line[len("OPTIM_AB "):]))
    print("| model | local step | best acc | final acc | ms/round |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['model']} | {r['row']} | {r['best_acc']:.4f} | "
              f"{r['final_acc']:.4f} | {r['ms_per_round']:.2f} |")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""BatchNorm vs GroupNorm A/B for ResNet-20 under the committee protocol.

Runs the fixed 8-client / committee-4 protocol on Dirichlet(0.3) shards
twice — norm_groups=0 (batch-stats BatchNorm) and norm_groups=8
(GroupNorm) — and prints, for each:

  ms/round        wall time of the timed rounds
  score spread    the committee's disagreement about ONE candidate: per
                  candidate max - min of its score over the scorers,
                  averaged over candidates and rounds
  test accuracy   sponsor evaluation after the same number of rounds

Each setting runs in a fresh child process under its own `timeout`, one
at a time; the first failure stops the script (no retries).

    python benchmarks/norm_ab.py [--rounds 30] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_setting(args, norm_groups: int) -> dict:
    import torch
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine

    assert torch.cuda.is_available(), "norm_ab needs a GPU"
    cfg = FLConfig.for_world(
        8, model="resnet20", n_class=10, norm_groups=norm_groups,
        samples_per_client=args.samples_per_client,
        batch_size=args.batch_size, partition="dirichlet",
        dirichlet_alpha=0.3, eval_samples=2 * args.samples_per_client,
        learning_rate=args.lr, max_epoch=args.rounds + args.warmup + 10)
    assert cfg.comm_count == 4
    t = Transport()
    shards, test = make_federated(cfg)
    eng = FLEngine(cfg, t, shards, test)

    # every scorer's score map passes through the "scores" gather: read
    # the per-candidate disagreement there, without touching the engine
    spreads = []
    gather = eng._gather

    def tap(phase, fn, *a):
        res = gather(phase, fn, *a)
        if phase == "scores":
            by_cand = {}
            for rank_scores in res:
                for _origin, smap, _tag in rank_scores:
                    for cand, s in smap.items():
                        by_cand.setdefault(cand, []).append(float(s))
            per = [max(v) - min(v) for v in by_cand.values() if len(v) > 1]
            if per:
                spreads.append(sum(per) / len(per))
        return res

    eng._gather = tap
    for _ in range(args.warmup):
        eng.run_round()
    torch.cuda.synchronize(t.device)
    n_warm = len(spreads)
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        eng.run_round()
    torch.cuda.synchronize(t.device)
    ms = (time.perf_counter() - t0) * 1e3 / args.rounds
    timed = spreads[n_warm:]
    acc = eng.evaluate_global()
    t.close()
    return {"norm_groups": norm_groups,
            "norm": "groupnorm" if norm_groups else "batchnorm",
            "ms_per_round": round(ms, 3),
            "score_spread": round(sum(timed) / max(len(timed), 1), 5),
            "test_acc": round(float(acc), 4),
            "rounds": args.rounds, "warmup": args.warmup,
            "samples_per_client": args.samples_per_client,
            "batch_size": args.batch_size}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples-per-client", type=int, default=1024)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed for each setting's child process")
    ap.add_argument("--run", type=int, default=None,
                    help="(child) run one setting with this norm_groups")
    args = ap.parse_args()
    if args.run is not None:
        print("NORM_AB " + json.dumps(run_setting(args, args.run)),
              flush=True)
        return
    passthrough = ["--rounds", args.rounds, "--warmup", args.warmup,
                   "--samples-per-client", args.samples_per_client,
                   "--batch-size", args.batch_size, "--lr", args.lr]
    for g in (0, args.groups):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable,
               os.path.abspath(__file__), "--run", str(g)] \
            + [str(a) for a in passthrough]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"norm_ab: norm_groups={g} exited with {rc}; "
                             "stopping")


if __name__ == "__main__":
    main()

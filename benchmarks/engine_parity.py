#!/usr/bin/env python3
"""Engine parity audit: pairwise tests (streams versus sequential, graph
versus eager) cannot see a change that shifts every path together, so a
refactor of the round engine is compared with its parent commit
directly. For each row of a fixed config matrix this builds an engine,
runs 4 rounds and prints ONE JSON line: the row, the mode, the sha256 of
the global model after every round, the selected origins per round, the
ledger roles at the end and n_updates per round. The loss is left out
on purpose: it accumulates through the one documented atomicAdd and is
not bitwise run to run on the GPU.

Run the SAME file on a checkout of the parent and on the branch and
diff the output; every line must be equal:

    python benchmarks/engine_parity.py --device cpu  > branch.txt
    python benchmarks/engine_parity.py --device cuda > branch_gpu.txt

On cuda every row runs in three modes — default (concurrent streams),
BFLC_STREAMS=0 and use_graphs=False — one child process per mode, since
the BFLC_* environment switches are read once per process.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 4
BASE = dict(model="mlp", n_features=32, n_class=8, samples_per_client=128,
            batch_size=64, eval_samples=128)
ROWS = [
    ("sgd", {}),
    ("adam", dict(optimizer="adam", learning_rate=0.001)),
    ("sgdm_ext", dict(momentum=0.9, lr_schedule="cosine", lr_total_rounds=6,
                      clip_norm=5.0, prox_mu=0.01)),
    ("dp_local", dict(dp_clip=0.5, dp_noise_multiplier=0.5)),
    ("dp_central", dict(dp_clip=0.5, dp_noise_multiplier=0.5,
                        dp_mode="central")),
    ("trimmed_mean", dict(aggregator="trimmed_mean")),
    ("byz_scale", dict(byzantine_clients=2, byzantine_attack="scale")),
    ("femnist_cnn", dict(model="femnist_cnn", n_class=62,
                         samples_per_client=256, batch_size=128,
                         eval_samples=256, partition="dirichlet")),
]
# mode -> (environment of the child, FLConfig overrides)
MODES = {
    "default": ({}, {}),
    "streams0": ({"BFLC_STREAMS": "0"}, {}),
    "eager": ({}, {"use_graphs": False}),
}


def run_rows(device: str, mode: str) -> None:
    import torch
    from bflc_amd.comm import Transport
    from bflc_amd.config import FLConfig
    from bflc_amd.data import make_federated
    from bflc_amd.fl import FLEngine
    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    for name, kw in ROWS:
        cfg = FLConfig.for_world(8, **{**BASE, **kw, **MODES[mode][1]})
        shards, test = make_federated(cfg)
        eng = FLEngine(cfg, Transport(device=dev), shards, test)
        shas, selected, n_updates = [], [], []
        for _ in range(ROUNDS):
            st = eng.run_round()
            shas.append(hashlib.sha256(
                eng.global_flat.cpu().numpy().tobytes()).hexdigest())
            selected.append([o for o, _ in eng.last_decision.selected])
            n_updates.append(st.n_updates)
        print(json.dumps({"row": name, "mode": mode, "global_sha256": shas,
                          "selected": selected,
                          "roles": sorted(eng.ledger.roles().items()),
                          "n_updates": n_updates}, sort_keys=True),
              flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", choices=["cpu", "cuda"], default="cpu")
    ap.add_argument("--mode", choices=sorted(MODES), default=None,
                    help="run one mode in this process (what the cuda "
                         "driver starts its children with)")
    ap.add_argument("--step-timeout", type=int, default=300,
                    help="seconds allowed per child process")
    args = ap.parse_args()
    if args.mode is not None or args.device == "cpu":
        run_rows(args.device, args.mode or "default")
        return
    for mode, (env, _) in MODES.items():
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable,
               os.path.abspath(__file__), "--device", "cuda", "--mode", mode]
        rc = subprocess.run(cmd, env={**os.environ, **env}).returncode
        if rc != 0:  # a failed child ends the audit: start nothing more
            raise SystemExit(f"engine_parity: mode {mode} exited {rc}")


if __name__ == "__main__":
    main()

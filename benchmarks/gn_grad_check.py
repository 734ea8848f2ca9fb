#!/usr/bin/env python3
"""Whole-model gradient check: ResNet-20 on the GPU (bf16 HIP kernels)
against the same model on the CPU (fp32 oracle ops), for BatchNorm
(norm_groups=0) and GroupNorm. Same init, same 64-sample batch; prints
both losses, the cosine of the two flat gradients and their norm ratio.

Separates "the kernels are wrong" from "this normalisation trains
differently": a kernel or wiring defect shows as a low cosine, a
property of the model shows on the CPU oracle as well.

    python benchmarks/gn_grad_check.py [--groups 8] [--batch 64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bflc_amd.config import FLConfig         # noqa: E402
from bflc_amd.models import build_model      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gn_grad_check needs a GPU"
    dev = torch.device("cuda", 0)
    for groups in (0, args.groups):
        cfg = FLConfig(model="resnet20", n_class=10, client_num=1,
                       comm_count=1, needed_update_count=1,
                       aggregate_count=1, norm_groups=groups)
        mg = build_model(cfg, dev)
        mc = build_model(cfg, torch.device("cpu"))
        torch.manual_seed(0)
        x = torch.randn(args.batch, 32, 32, 3)
        y = torch.randint(0, 10, (args.batch,))
        lg = mg.loss(x, y.to(dev))
        lg.backward()
        lc = mc.loss(x, y)
        lc.backward()
        gg = mg.grad_flat().float().cpu()
        gc = mc.grad_flat()
        cos = torch.nn.functional.cosine_similarity(gg, gc, dim=0)
        print(f"norm_groups={groups} loss gpu {float(lg.detach()):.4f} "
              f"cpu {float(lc.detach()):.4f} grad cosine {float(cos):.5f} "
              f"norm ratio {float(gg.norm() / gc.norm()):.4f}", flush=True)


if __name__ == "__main__":
    main()

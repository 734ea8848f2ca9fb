"""One smallest case per GEMM launcher family, compared BITWISE against
outputs recorded on an MI355X at the commit before the launchers were
rewritten around the shared planner (tests/golden/
gemm_dispatch_parent.npz; inputs regenerated exactly by det()). Each
test also asserts, through the route queries, that its shape takes the
launcher it is meant to pin.

Run as a script, `--dump FILE` computes the same cases and writes them
as an .npz: the golden file was recorded that way, and the
BFLC_WGRAD_KPAIR=0 test uses it to compute its case in a fresh child
process (the gate is read once per process).
"""
import argparse
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden" / "gemm_dispatch_parent.npz"

TT = [(False, False), (False, True), (True, False), (True, True)]
# (M, K, N); the second has N % 8 != 0, so the scalar staging flags run
GEMM_RAW = {"m100_k40_n24": (100, 40, 24), "m33_k72_n62": (33, 72, 62)}
SPLITK = (32, 4096, 64)        # small tile, K split
WGRAD_DENSE = (64, 4096, 128)  # ta, !tb: routed to the small kernel
# smallest M = N multiple of 256 that gemm_plan_route sends to gemm8p
# at K = 512 (below it the cost model prefers the 64- and 128-row
# gemm256 tiles, which fill the chip better); its 25 MB output is
# recorded as digest()
GEMM8P = (3584, 512, 3584)
# name: (N, H, W, C, Kout) — 3x3, stride 1, pad 1
CONV = {
    "n8_8x8_c32_k64": (8, 8, 8, 32, 64),   # wide-N forward, implicit bwd
    "n4_8x8_c16_k16": (4, 8, 8, 16, 16),   # narrow-N forward and backward
}
CONV_STATS_ONLY = {"n41_12x12_c32_k64": (41, 12, 12, 32, 64)}  # S = 1
COLSUM = [(100, 62), (100, 10), (5000, 64)]
RELU_COLSUM = (5000, 64)


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def det(shape, seed, scale):
    """Machine-independent pseudo-random tensor: integer hash -> k*scale,
    |k| <= 127 and scale a power of two, so every value is exact in
    bf16 on any host."""
    n = math.prod(shape)
    i = torch.arange(n, dtype=torch.int64)
    h = (i * 2654435761 + seed * 40503 + 12345) % 2147483647
    k = (h >> 7) % 255 - 127
    return (k.to(torch.float32) * scale).reshape(shape)


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def gemm_raw(m, k, n, ta, tb, seed):
    a = bf(det((k, m) if ta else (m, k), seed, 1.0 / 64))
    b = bf(det((n, k) if tb else (k, n), seed + 1, 1.0 / 1024))
    return hip().gemm_raw(a, b, ta, tb)


def digest(t):
    """Position-weighted int64 checksums of a bf16 matrix's bit pattern,
    one per row then one per column: any changed element changes both."""
    b = t.view(torch.int16).to(torch.int64)
    r = torch.arange(1, b.shape[0] + 1, device=b.device).unsqueeze(1)
    c = torch.arange(1, b.shape[1] + 1, device=b.device).unsqueeze(0)
    return torch.cat([(b * c).sum(1), (b * r).sum(0)])


def conv_tensors(case):
    n, h, w, c, kout = case
    x = bf(det((n, h, w, c), 1, 1.0 / 64))
    wt = bf(det((kout, 3, 3, c), 2, 1.0 / 1024))
    dy = bf(det((n, h, w, kout), 3, 1.0 / 256))
    return x, wt, dy


def relu_colsum_inputs():
    m, n = RELU_COLSUM
    return bf(det((m, n), 51, 1.0 / 64)), bf(det((m, n), 52, 1.0 / 256))


def compute(group):
    """{key: tensor} of one group of cases."""
    out = {}
    if group == "gemm_raw":
        for name, (m, k, n) in GEMM_RAW.items():
            for ta, tb in TT:
                out[f"gemm_raw.{name}.ta{int(ta)}tb{int(tb)}"] = gemm_raw(
                    m, k, n, ta, tb, 11)
        out["splitk"] = gemm_raw(*SPLITK, False, False, 13)
        out["wgrad_dense"] = gemm_raw(*WGRAD_DENSE, True, False, 15)
        out["gemm8p.digest"] = digest(gemm_raw(*GEMM8P, False, True, 17))
    elif group == "conv_bwd":
        for name, case in CONV.items():
            x, wt, dy = conv_tensors(case)
            dx, dw, db = hip().conv2d_bwd(x, wt, dy, 1, 1, None, True, True)
            out.update({f"conv_bwd.{name}.dx": dx, f"conv_bwd.{name}.dw": dw,
                        f"conv_bwd.{name}.db": db})
    elif group == "conv_fwd_bn":
        for name, case in {**CONV, **CONV_STATS_ONLY}.items():
            x, wt, _ = conv_tensors(case)
            y, _, psum, psq = hip().conv2d_fwd_bn(x, wt, 1, 1)
            if name in CONV:
                out[f"conv_fwd_bn.{name}.y"] = y
            out[f"conv_fwd_bn.{name}.psum"] = psum
            out[f"conv_fwd_bn.{name}.psq"] = psq
    elif group == "colsum":
        for m, n in COLSUM:  # linear_bwd's db is colsum_bf16(dy)
            x = bf(det((m, 8), 41, 1.0 / 64))
            w = bf(det((8, n), 42, 1.0 / 1024))
            dy = bf(det((m, n), 43, 1.0 / 256))
            out[f"colsum.m{m}_n{n}"] = hip().linear_bwd(x, w, dy, False)[2]
        y, dy = relu_colsum_inputs()
        out["relu_bwd_colsum.db"] = hip().relu_bwd_colsum(y, dy)[1]
    else:
        raise ValueError(group)
    return out


GROUPS = ["gemm_raw", "conv_bwd", "conv_fwd_bn", "colsum"]


def as_bits(t):
    """Raw bit pattern as a flat numpy array (bf16 -> int16)."""
    t = t.detach().contiguous().cpu().reshape(-1)
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.numpy()


def dump(path, groups, prefix=""):
    arrays = {}
    for g in groups:
        for k, v in compute(g).items():
            arrays[prefix + k] = as_bits(v)
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


def check_group(group, golden, prefix=""):
    got = compute(group)
    assert got
    for k, v in got.items():
        ref = golden[prefix + k]
        bits = as_bits(v)
        assert bits.dtype == ref.dtype and bits.shape == ref.shape, k
        assert np.array_equal(bits, ref), k


def test_dense_routes():
    q = hip().gemm_plan_route
    for m, k, n in GEMM_RAW.values():
        for ta, tb in TT:
            assert q(m, n, k, ta, tb)[0] == "small"
    m, k, n = SPLITK
    path, _, _, s, kslice = q(m, n, k, False, False)
    assert path == "small" and s > 1 and kslice * s >= k
    m, k, n = WGRAD_DENSE
    assert q(m, n, k, True, False)[0] == "small"
    assert q(m, n, k, False, True)[0] != "small"  # the layout decides
    m, k, n = GEMM8P
    assert q(m, n, k, False, True)[0] == "gemm8p"
    for smaller in range(256, m, 256):
        assert q(smaller, smaller, k, False, True)[0] != "gemm8p"


def test_conv_routes():
    q = hip().conv_plan_route
    for name, (n, h, w, c, kout) in {**CONV, **CONV_STATS_ONLY}.items():
        xs, ws = [n, h, w, c], [kout, 3, 3, c]
        fwd = q("fwd", xs, ws, 1, 1)
        assert fwd[0] == ("gemm256" if kout % 64 == 0 else "small"), name
        assert q("dgrad", xs, ws, 1, 1)[0] == "small", name  # N = C < 64
        wg = q("wgrad", xs, ws, 1, 1)
        assert wg[0] == "small" and wg[3] > 1, name
    # the stats epilogue only runs unsplit
    n, h, w, c, kout = CONV_STATS_ONLY["n41_12x12_c32_k64"]
    assert q("fwd", [n, h, w, c], [kout, 3, 3, c], 1, 1)[3] == 1


@pytest.mark.parametrize("group", GROUPS)
def test_matches_recorded(group, golden):
    check_group(group, golden)


def test_conv_fwd_bn_stats_present(golden):
    """The unsplit shape really carries epilogue partials."""
    assert golden["conv_fwd_bn.n41_12x12_c32_k64.psum"].size > 0


def test_relu_bwd_colsum_dx_exact():
    y, dy = relu_colsum_inputs()
    dx = hip().relu_bwd_colsum(y, dy)[0]
    assert torch.equal(dx, torch.where(y.float() > 0, dy, torch.zeros_like(dy)))


def test_conv_bwd_kpair_off_matches_recorded(golden, tmp_path):
    """BFLC_WGRAD_KPAIR=0 (the scatter staging without k pairs) in a
    fresh process, against what that gate gave at the parent."""
    out = tmp_path / "kpair0.npz"
    env = dict(os.environ, BFLC_WGRAD_KPAIR="0",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--dump", str(out), "--groups",
                    "conv_bwd", "--prefix", "kpair0."],
                   check=True, env=env, timeout=300)
    with np.load(out) as z:
        keys = list(z.files)
        assert keys
        for k in keys:
            assert np.array_equal(z[k], golden[k]), k


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    ap.add_argument("--groups", nargs="+", default=GROUPS)
    ap.add_argument("--prefix", default="")
    a = ap.parse_args()
    dump(a.dump, a.groups, a.prefix)

"""Halo-tile data gradient of conv2's pooled backward, bitwise.

halo_pool_dgrad_kernel unpools the pooled (dy, y, idx) into zero-ringed
LDS images, writes the masked full-resolution plane for the weight
gradient and runs the unsplit implicit dgrad's MFMA chain (from +0, 18
chunks ascending in k = (r*3+s)*64 + kout) into its plain epilogue. The
oracle is the parent chain on the same inputs

    pool_relu_bwd_colsum(y, idx, dy)      -> plane, db
    conv2d_bwd(x, w, plane, 1, 1, None, False, True) -> dx, dw

and every comparison is torch.equal, no tolerance.

The route only takes shapes whose dgrad plan has one K slice, and every
small batch plans split-K, so one oracle per (H, W) is computed once on
the smallest power-of-two batch that plans S == 1 (asked through
conv_plan_route) and never written to afterwards. A small case runs its
own N images, the first N of that batch, through the pinned kernel
against the oracle's first N images: a row's chain does not depend on
the batch around it.

BFLC_HALO_DGRAD is read once per process, so the gate-off side of the
model-level comparison runs in a fresh child process, once per module.
"""
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
C, KOUT = 32, 64
W_SHAPE = [KOUT, 3, 3, C]
MODEL_BATCH = 96
NAMES = ["c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b"]


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def group_images(h, w):
    """G: images the kernel unpools per LDS group at this geometry."""
    return hip().halo_dgrad_group_images([1, h, w, C], W_SHAPE, 1, 1)


def dgrad_plan(n, h, w):
    return hip().conv_plan_route("dgrad", [n, h, w, C], W_SHAPE, 1, 1)


def unsplit_batch(h, w):
    """Smallest power-of-two batch whose dgrad plans one K slice."""
    n = 1
    while True:
        path, _, _, s, _ = dgrad_plan(n, h, w)
        if path != "none" and s == 1:
            return n
        n *= 2
        assert n <= 1 << 16, (h, w)


def rand_inputs(n, h, w, seed):
    """Asymmetric weights; half the channels get a bias low enough that
    many pool windows are all zero after ReLU (ties -> idx 0). dy has
    exact +0 and -0 elements."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, C, generator=g)
    wt = torch.randn(KOUT, 3, 3, C, generator=g) / math.sqrt(9 * C)
    b = torch.randn(KOUT, generator=g) * 0.5
    b[::2] -= 1.5
    dy = torch.randn(n, h // 2, w // 2, KOUT, generator=g)
    u = torch.rand(dy.shape, generator=g)
    dy[u < 0.05] = 0.0
    dy[u > 0.92] = -0.0
    return bf(x), bf(wt), bf(b), bf(dy)


def is_neg_zero(t):
    return t.view(torch.int16) == -32768


def parent_chain(x, wt, yp, idx, dy):
    """(plane, dx, dw, db) of the unpool kernel and conv2d_bwd."""
    n, h, w = x.shape[0], x.shape[1], x.shape[2]
    plane, db = hip().pool_relu_bwd_colsum(yp, idx, dy, [n, h, w, KOUT])
    dx, dw, _ = hip().conv2d_bwd(x, wt, plane, 1, 1, None, False, True)
    return plane, dx, dw, db


def check_oracle_inputs(yp, idx, dy):
    dead = (yp == 0)
    frac = dead.float().mean().item()
    assert 0.1 < frac < 0.95, frac
    for code in range(4):
        assert (idx == code).any(), code
    assert (is_neg_zero(dy) & (yp > 0)).any()


_ORACLE = {}


def oracle(h, w):
    """Inputs and parent results of the unsplit batch at (h, w): computed
    once per geometry and never written to afterwards."""
    key = (h, w)
    if key not in _ORACLE:
        nb = unsplit_batch(h, w)
        x, wt, b, dy = rand_inputs(nb, h, w, seed=1000 * h + w)
        yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1)
        check_oracle_inputs(yp, idx, dy)
        plane, dx, dw, db = parent_chain(x, wt, yp, idx, dy)
        _ORACLE[key] = dict(x=x, w=wt, yp=yp, idx=idx, dy=dy, plane=plane,
                            dx=dx, dw=dw, db=db)
    return _ORACLE[key]


_STALE = {}


def stale_oracle(h, w):
    """The oracle batch with the argmax codes set by hand: image i of
    group j carries code (base + j) % 4 at every window, so a position
    selected in one group is unselected in the next."""
    key = (h, w)
    if key not in _STALE:
        o = oracle(h, w)
        g = group_images(h, w)
        assert g >= 1
        nb = o["x"].shape[0]
        gen = torch.Generator().manual_seed(77)
        base = torch.randint(0, 4, (1,) + tuple(o["idx"].shape[1:]),
                             generator=gen)
        grp = (torch.arange(nb) // g).view(nb, 1, 1, 1)
        idx = ((base + grp) % 4).to(torch.uint8).to(DEV).contiguous()
        step = g * idx[0].numel()
        flat = idx.view(-1)
        assert (flat[step:] != flat[:-step]).all()
        check_oracle_inputs(o["yp"], idx, o["dy"])
        plane, dx, dw, db = parent_chain(o["x"], o["w"], o["yp"], idx,
                                         o["dy"])
        _STALE[key] = dict(o, idx=idx, plane=plane, dx=dx, dw=dw, db=db)
    return _STALE[key]


def assert_pinned(o, n, max_blocks):
    yp, idx, dy = (o[k][:n].contiguous() for k in ("yp", "idx", "dy"))
    for _ in range(2):
        dx, plane = hip().halo_pool_dgrad(o["w"], yp, idx, dy, max_blocks)
        assert torch.equal(plane, o["plane"][:n])
        assert torch.equal(dx, o["dx"][:n])
        # the signs of the zeros as well
        assert torch.equal(plane.view(torch.int16),
                           o["plane"][:n].view(torch.int16))


# (N, H, W): every tap but the centre in the ring | tiles cross images |
# workload geometry, N below a block's share | N no multiple of G at any
# geometry with G > 1, several groups | non-square
CASES = [(1, 2, 2), (5, 6, 6), (3, 14, 14), (9, 14, 14), (3, 6, 10),
         (23, 2, 2), (7, 6, 6)]


@pytest.mark.parametrize("max_blocks", [0, 1], ids=["grid", "oneblock"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_pinned_bitwise(case, max_blocks):
    n, h, w = case
    assert group_images(h, w) >= 1
    assert_pinned(oracle(h, w), n, max_blocks)


def test_without_plane_store():
    """store_plane=False (the measurement variant): same dx, no plane."""
    o = oracle(14, 14)
    n = 5
    yp, idx, dy = (o[k][:n].contiguous() for k in ("yp", "idx", "dy"))
    dx, plane = hip().halo_pool_dgrad(o["w"], yp, idx, dy, 2, False)
    assert plane.numel() == 0
    assert torch.equal(dx, o["dx"][:n])


def test_unsplit_batches():
    """The oracle batches at the two main geometries: dgrad plans one K
    slice from 50 images at 14x14 and from 269 at 6x6."""
    assert unsplit_batch(14, 14) == 64
    assert unsplit_batch(6, 6) == 512


def test_largest_geometry():
    """(2, 22, 22): run it if the LDS gate takes it, else the query and
    the pinned entry must both decline."""
    h = w = 22
    if group_images(h, w) >= 1:
        for mb in (0, 1):
            assert_pinned(oracle(h, w), 2, mb)
        return
    nb = unsplit_batch(h, w)
    assert hip().pool_dgrad_impl([nb, h, w, C], W_SHAPE, 1, 1,
                                 True) == "implicit_gemm"
    x, wt, b, dy = rand_inputs(2, h, w, seed=3)
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1)
    with pytest.raises(RuntimeError):
        hip().halo_pool_dgrad(wt, yp, idx, dy, 0)
    with pytest.raises(RuntimeError):
        hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, 1, True, True,
                                   True, "halo_mfma")


@pytest.mark.parametrize("hw", [(14, 14), (6, 6)],
                         ids=lambda c: "x".join(map(str, c)))
def test_stale_lds(hw):
    """One block walks consecutive groups whose argmax codes differ at
    every window: what a group does not select must be rewritten as
    zeros, LDS still holds the previous group's values there."""
    h, w = hw
    o = stale_oracle(h, w)
    g = group_images(h, w)
    assert_pinned(o, min(o["x"].shape[0], 4 * g + 1), 1)


def test_default_route():
    o = oracle(14, 14)
    xs = list(o["x"].shape)
    assert hip().conv2d_relu_pool_bwd_route(xs, W_SHAPE, 1, 1, True,
                                            True) == "unpool"
    assert hip().pool_dgrad_impl(xs, W_SHAPE, 1, 1, True) == "halo_mfma"
    for _ in range(2):
        dx, dw, db = hip().conv2d_relu_pool_bwd(
            o["x"], o["w"], o["yp"], o["idx"], o["dy"], 1, 1, True, True)
        assert torch.equal(dx, o["dx"])
        assert torch.equal(dw, o["dw"])
        assert torch.equal(db, o["db"])


@pytest.mark.parametrize("impl", ["halo_mfma", "implicit_gemm"])
def test_pinned_route(impl):
    """Either implementation pinned through the backward entry."""
    o = oracle(14, 14)
    dx, dw, db = hip().conv2d_relu_pool_bwd(
        o["x"], o["w"], o["yp"], o["idx"], o["dy"], 1, 1, True, True, True,
        impl, 3)
    assert torch.equal(dx, o["dx"])
    assert torch.equal(dw, o["dw"])
    assert torch.equal(db, o["db"])


def test_gate_split_k():
    """A 14x14 batch of 32 plans two K slices: the old kernels stay."""
    n, h, w = 32, 14, 14
    path, _, _, s, _ = dgrad_plan(n, h, w)
    assert path != "none" and s == 2
    assert hip().pool_dgrad_impl([n, h, w, C], W_SHAPE, 1, 1,
                                 True) == "implicit_gemm"
    x, wt, b, dy = rand_inputs(n, h, w, seed=21)
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1)
    _, dx_ref, dw_ref, db_ref = parent_chain(x, wt, yp, idx, dy)
    dx, dw, db = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, 1, True,
                                            True)
    assert torch.equal(dx, dx_ref)
    assert torch.equal(dw, dw_ref)
    assert torch.equal(db, db_ref)


def test_gate_no_dx():
    o = oracle(14, 14)
    xs = list(o["x"].shape)
    assert hip().pool_dgrad_impl(xs, W_SHAPE, 1, 1, False) == "implicit_gemm"
    dx, dw, db = hip().conv2d_relu_pool_bwd(
        o["x"], o["w"], o["yp"], o["idx"], o["dy"], 1, 1, True, False)
    assert dx.numel() == 0
    assert torch.equal(dw, o["dw"])
    assert torch.equal(db, o["db"])


# ------------------------------------------------------------ model level

def model_grads(batch):
    """One training step's gradients of FemnistCNN."""
    from bflc_amd.config import FLConfig
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, model="femnist_cnn", n_class=62,
                             samples_per_client=64, batch_size=32,
                             eval_samples=64)
    m = build_model(cfg, torch.device(DEV))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # non-zero biases
        m.flat.add_(0.05 * torch.randn(m.numel, generator=g).to(DEV))
    m._sync_shadow()
    x = bf(torch.randn(batch, 28, 28, 1, generator=g))
    y = torch.randint(0, 62, (batch,), generator=g).to(DEV)
    m.zero_grad()
    m.loss(x, y).backward()
    return {f"grad.{k}": m.p(k).grad.detach().clone() for k in NAMES}


def as_bits(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy()


def conv2_dgrad_impl(batch):
    return hip().pool_dgrad_impl([batch, 14, 14, C], W_SHAPE, 1, 1, True)


def child_main(out):
    res = {"impl": np.array(conv2_dgrad_impl(MODEL_BATCH))}
    for k, v in model_grads(MODEL_BATCH).items():
        res[k] = as_bits(v)
    np.savez(out, **res)


@pytest.fixture(scope="module")
def gate_off(tmp_path_factory):
    out = tmp_path_factory.mktemp("halo_dgrad") / "gate_off.npz"
    env = dict(os.environ, BFLC_HALO_DGRAD="0", BFLC_FUSED_POOL="1",
               BFLC_FUSED_POOL_TRAIN="1",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--child", str(out)],
                   check=True, env=env, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_femnist_cnn_gate_on_vs_off(gate_off, monkeypatch):
    """All eight gradients of one step at batch 96, gate on (this
    process) against BFLC_HALO_DGRAD=0 (the child): bitwise."""
    monkeypatch.setenv("BFLC_FUSED_POOL", "1")
    monkeypatch.setenv("BFLC_FUSED_POOL_TRAIN", "1")
    assert str(gate_off["impl"]) == "implicit_gemm"
    assert conv2_dgrad_impl(MODEL_BATCH) == "halo_mfma"
    outs = model_grads(MODEL_BATCH)
    for k, v in outs.items():
        assert v.float().abs().sum() > 0, k
        assert np.array_equal(as_bits(v), gate_off[k]), k


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])

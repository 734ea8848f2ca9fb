"""Every reachable GEMM and implicit-conv plan against an exact oracle.

The cases of gemm_exact_cases.py (one smallest shape per launch-plan
class, plus the plans named one by one there) run on the GPU and must
equal the float64 result rounded once to bf16, BITWISE: the inputs are
built so that fp32 accumulation in any order is exact, which leaves the
final store as the kernels' only rounding (see that module's docstring).

One test per group. Each loops over its cases, asserts through the
route query that the case still takes the class it is listed under,
collects the class key of every case with a mismatching element and
asserts that the list is empty. Wall times are printed, not asserted.

Run as a script, `--dump FILE` computes the implicit-wgrad cases and
writes their bit patterns as an .npz: the BFLC_WGRAD_KPAIR=0 test uses
it to run them in a fresh child process (the gate is read once per
process).
"""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

import gemm_exact_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = Path(__file__).resolve().parent.parent
ROW_CHUNK = 1 << 20  # oracle rows per step for the multi-million-row cases


def hip():
    return gc.hip()


def dev(t):
    return t.to(DEV).contiguous()


class Group:
    """Collects the failing class keys of one group and its wall time."""

    def __init__(self, name):
        self.name, self.bad, self.n = name, [], 0
        self.t0 = time.perf_counter()

    def check(self, key, got, want, what=""):
        self.n += 1
        nbad = gc.mismatches(got.cpu(), want)
        if nbad:
            self.bad.append((tuple(key), what, nbad, want.numel()))

    def done(self):
        torch.cuda.synchronize()
        print(f"\n[exact] {self.name}: {self.n} comparisons, "
              f"{len(self.bad)} failing, {time.perf_counter() - self.t0:.2f} s")
        for entry in self.bad:
            print("[exact]   mismatch:", entry)
        assert self.n > 0
        assert self.bad == [], self.bad[:10]


def dense_operands(c, seed, bias=False):
    """(a, b, bias) of a dense case in its storage layout, amplitudes
    from K so that the exactness bound holds."""
    bias_units = gc.BIAS_UNITS if bias else 0
    amp_a, amp_b = gc.pick_amps(c.k, bias_units)
    gc.assert_bound(amp_a, amp_b, c.k, bias_units)
    a = gc.ints((c.k, c.m) if c.ta else (c.m, c.k), amp_a, seed, gc.SCALE_A)
    b = gc.ints((c.n, c.k) if c.tb else (c.k, c.n), amp_b, seed + 1,
                gc.SCALE_B)
    bv = gc.ints((c.n,), gc.BIAS_AMP, seed + 2, gc.SCALE_BIAS) if bias \
        else None
    return a, b, bv


def assert_dense_route(c):
    assert gc.dense_case(*c[:5]).key == c.key, c


def assert_conv_route(c):
    assert gc.conv_case(c.entry, c.shape).key == c.key, c


@pytest.mark.parametrize("path", ["small", "gemm256", "gemm8p"])
def test_gemm_raw(path):
    """gemm_raw in all four layouts. The double-buffered cases with ta
    or !tb go through transpose_bf16 first, at dimensions that are no
    multiple of its 64 x 64 tile."""
    g = Group(f"gemm_raw/{path}")
    cases = [c for c in gc.dense_cases() if c.key.path == path]
    assert cases
    for i, c in enumerate(cases):
        assert_dense_route(c)
        a, b, _ = dense_operands(c, 10 * i + 1)
        got = hip().gemm_raw(dev(a), dev(b), c.ta, c.tb)
        g.check(c.key, got, gc.matmul_oracle(a, b, c.ta, c.tb))
    g.done()


def test_linear_fwd():
    """Bias and bias + ReLU epilogues of every kernel family, unsplit
    (in the GEMM's own epilogue) and split (in either reduce kernel)."""
    g = Group("linear_fwd")
    cases = gc.linear_fwd_cases()
    kinds = {(c.key.path, c.key.reduce) for c in cases}
    for path in ("small", "gemm256", "gemm8p"):
        assert {(path, None), (path, "vec")} <= kinds, kinds
    assert {("small", r) for r in ("tree<=8", "tree9-32", "tree>32")} <= kinds
    for i, c in enumerate(cases):
        assert_dense_route(c)
        x, w, b = dense_operands(c, 10 * i + 3, bias=True)
        acc = x.double() @ w.double()
        xd, wd, bd = dev(x), dev(w), dev(b)
        for relu in (False, True):
            got = hip().linear_fwd(xd, wd, bd, relu)
            g.check(c.key, got, gc.round_once(acc, b, relu), f"relu={relu}")
    g.done()


def test_linear_bwd():
    """dx and dw of linear_bwd (db: the tolerance tests of
    test_ops_gpu.py and the recorded colsum outputs cover it; a column
    sum of bf16 values is not a GEMM plan)."""
    g = Group("linear_bwd")
    for i, ((m, k, n), dx_plan, dw_plan) in enumerate(gc.LINEAR_BWD):
        assert gc.linear_bwd_routes(m, k, n) == (dx_plan, dw_plan), (m, k, n)
        # dy meets w over N (dx) and x over M (dw): both bounds must hold
        amp_dy, amp_w = gc.pick_amps(n)
        amp_x = max(a for a in (127, 15, 3, 1)
                    if a * amp_dy * m < gc.BOUND)
        gc.assert_bound(amp_dy, amp_w, n)
        gc.assert_bound(amp_x, amp_dy, m)
        x = gc.ints((m, k), amp_x, 10 * i + 5, gc.SCALE_A)
        w = gc.ints((k, n), amp_w, 10 * i + 6, gc.SCALE_B)
        dy = gc.ints((m, n), amp_dy, 10 * i + 7, gc.SCALE_DY)
        dx, dw, _ = hip().linear_bwd(dev(x), dev(w), dev(dy), True)
        g.check(("linear_bwd.dx", m, k, n) + dx_plan, dx,
                gc.matmul_oracle(dy, w, False, True))
        g.check(("linear_bwd.dw", m, k, n) + dw_plan, dw,
                gc.matmul_oracle(x, dy, True, False))
    g.done()


def test_thin_dense():
    """The thin kernels at all four KT, below and above the grid cap
    (16384 blocks of 256 rows): the larger M walks the grid-stride loop
    and ends in a ragged block."""
    g = Group("thin dense")
    for i, c in enumerate(gc.thin_cases()):
        assert_dense_route(c)
        a, b, _ = dense_operands(c, 10 * i + 2)
        got = hip().gemm_raw(dev(a), dev(b), False, True).cpu()
        assert got.shape == (c.m, c.n)
        nbad = 0
        for r0 in range(0, c.m, ROW_CHUNK):
            want = gc.matmul_oracle(a[r0:r0 + ROW_CHUNK], b, False, True)
            nbad += gc.mismatches(got[r0:r0 + ROW_CHUNK], want)
        g.n += 1
        if nbad:
            g.bad.append((tuple(c.key), c.m, nbad))
    g.done()


def conv_fwd_operands(shape, seed, bias):
    n, h, w, c, kout, r, stride, pad = shape
    bias_units = gc.BIAS_UNITS if bias else 0
    amp_x, amp_w = gc.pick_amps(r * r * c, bias_units)
    gc.assert_bound(amp_x, amp_w, r * r * c, bias_units)
    x = gc.ints((n, h, w, c), amp_x, seed, gc.SCALE_A)
    wt = gc.ints((kout, r, r, c), amp_w, seed + 1, gc.SCALE_B)
    b = gc.ints((kout,), gc.BIAS_AMP, seed + 2, gc.SCALE_BIAS) if bias \
        else None
    return x, wt, b


def test_conv2d_fwd():
    """conv2d_fwd on the implicit entry, with bias and bias + ReLU, and
    the thin conv forward past its grid cap (no route query names the
    thin conv kernel: that it runs rests on conv2d_fwd_col's gate, see
    conv_entry_taken)."""
    g = Group("conv2d_fwd")
    cases = list(gc.conv_cases("fwd"))
    thin = gc.ConvCase("fwd", gc.THIN_CONV, ("thin_conv", 16))
    assert gc.conv_route("fwd", gc.THIN_CONV)[0] == "none"
    for i, c in enumerate(cases + [thin]):
        if c is not thin:
            assert_conv_route(c)
        stride, pad = c.shape[6:]
        x, wt, b = conv_fwd_operands(c.shape, 10 * i + 1, bias=True)
        acc = gc.conv_fwd_acc(x, wt, stride, pad)
        xd, wd, bd = dev(x), dev(wt), dev(b)
        for relu in (False, True):
            got = hip().conv2d_fwd(xd, wd, bd, stride, pad, relu)
            g.check(c.key, got, gc.round_once(acc, b, relu), f"relu={relu}")
    g.done()


def conv_bwd_operands(c, seed):
    """(x, w, dy) of a dgrad or wgrad case. dy meets w over R*S*Kout in
    the dgrad and x over N*OH*OW in the wgrad; the case's own GEMM gets
    amplitudes inside the bound, the operand it does not read is small."""
    n, h, w, cin, kout, r, stride, pad = c.shape
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w + 2 * pad - r) // stride + 1
    k = gc.conv_dims(c.entry, *c.shape)[2]
    amp_dy, amp_o = gc.pick_amps(k)
    gc.assert_bound(amp_dy, amp_o, k)
    amp_x, amp_w = (amp_o, 1) if c.entry == "wgrad" else (1, amp_o)
    x = gc.ints((n, h, w, cin), amp_x, seed, gc.SCALE_A)
    wt = gc.ints((kout, r, r, cin), amp_w, seed + 1, gc.SCALE_B)
    dy = gc.ints((n, oh, ow, kout), amp_dy, seed + 2, gc.SCALE_DY)
    return x, wt, dy


def run_wgrad(c, seed):
    """(dw from the GPU, x, w, dy on the host) of a wgrad case."""
    stride, pad = c.shape[6:]
    x, wt, dy = conv_bwd_operands(c, seed)
    dw = hip().conv2d_bwd(dev(x), dev(wt), dev(dy), stride, pad, None,
                          False, False)[1]
    return dw, x, wt, dy


def test_conv2d_bwd():
    """dx and dw of conv2d_bwd, only at shapes the implicit dgrad /
    wgrad entries take (gemm_exact_cases.conv_entry_taken): the dcol +
    col2im fallback rounds twice by design — dcol to bf16, then the
    col2im sum — so it cannot equal a once-rounded oracle. Which entry
    conv2d_bwd takes is known here only through a copy of its gates
    (see conv_entry_taken for what that leaves unchecked)."""
    g = Group("conv2d_bwd")
    for i, c in enumerate(gc.conv_cases("dgrad")):
        assert_conv_route(c)
        stride, pad = c.shape[6:]
        x, wt, dy = conv_bwd_operands(c, 10 * i + 1)
        dx = hip().conv2d_bwd(dev(x), dev(wt), dev(dy), stride, pad, None,
                              False, True)[0]
        g.check(c.key, dx, gc.conv_bwd_oracle(x, wt, dy, stride, pad, 0))
    for i, c in enumerate(gc.conv_cases("wgrad")):
        assert_conv_route(c)
        dw, x, wt, dy = run_wgrad(c, 10 * i + 4)
        stride, pad = c.shape[6:]
        g.check(c.key, dw, gc.conv_bwd_oracle(x, wt, dy, stride, pad, 1))
    g.done()


def dump_wgrad(path):
    arrays = {}
    for i, c in enumerate(gc.conv_cases("wgrad")):
        dw = run_wgrad(c, 10 * i + 4)[0]
        arrays[f"dw{i}"] = dw.contiguous().cpu().view(torch.int16).numpy()
    np.savez_compressed(path, **arrays)


def test_wgrad_kpair_off(tmp_path):
    """BFLC_WGRAD_KPAIR=0 (the scatter staging without k pairs): the
    same wgrad cases computed in a fresh child process."""
    g = Group("wgrad, BFLC_WGRAD_KPAIR=0")
    out = tmp_path / "kpair0.npz"
    env = dict(os.environ, BFLC_WGRAD_KPAIR="0",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--dump", str(out)],
                   check=True, env=env, timeout=300)
    cases = gc.conv_cases("wgrad")
    with np.load(out) as z:
        assert len(z.files) == len(cases)
        for i, c in enumerate(cases):
            assert_conv_route(c)
            stride, pad = c.shape[6:]
            x, wt, dy = conv_bwd_operands(c, 10 * i + 4)
            want = gc.conv_bwd_oracle(x, wt, dy, stride, pad, 1)
            got = torch.from_numpy(z[f"dw{i}"]).view(torch.bfloat16)
            g.check(c.key, got.reshape(want.shape), want)
    g.done()


def test_conv2d_fwd_bn():
    """conv2d_fwd_bn: y bitwise; the fused per-tile-row BN partials, on
    every unsplit plan, against float64 sums of the oracle's bf16 y over
    the same bm rows. The partials are fp32 sums of bm values (v, or the
    exact fp32 product v * v) in a fixed tree: each of the bm - 1 adds
    rounds by at most 2^-24 of a partial sum no larger than sum|v|,
    hence |psum - sum v| <= (bm - 1) * 2^-24 * sum|v|, and the same
    with v^2 for psq. Derived, not tuned."""
    g = Group("conv2d_fwd_bn")
    stats_bad, n_stats = [], 0
    for i, c in enumerate(gc.conv_cases("fwd")):
        assert_conv_route(c)
        stride, pad = c.shape[6:]
        x, wt, _ = conv_fwd_operands(c.shape, 10 * i + 1, bias=False)
        want = gc.conv_fwd_oracle(x, wt, stride, pad)
        y, _, psum, psq = hip().conv2d_fwd_bn(dev(x), dev(wt), stride, pad)
        g.check(c.key, y, want, "y")
        if c.key.split:  # the stats epilogue only runs unsplit
            assert psum.numel() == 0 and psq.numel() == 0, c
            continue
        m, n, _ = gc.conv_dims("fwd", *c.shape)
        bm = c.key.bm
        chunks = -(-m // bm)
        assert psum.shape == (chunks, n) and psq.shape == (chunks, n), c
        v = torch.zeros(chunks * bm, n, dtype=torch.float64)
        v[:m] = want.reshape(m, n).double()
        v = v.reshape(chunks, bm, n)
        eps = (bm - 1) * 2.0 ** -24
        for name, part, val in (("psum", psum, v), ("psq", psq, v * v)):
            err = (part.cpu().double() - val.sum(1)).abs()
            bound = eps * val.abs().sum(1)
            n_stats += 1
            if bool((err > bound).any()):
                stats_bad.append((tuple(c.key), name,
                                  float((err - bound).max())))
    assert n_stats > 0
    assert stats_bad == [], stats_bad[:10]
    g.done()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True)
    dump_wgrad(ap.parse_args().dump)

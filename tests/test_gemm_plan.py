"""The GEMM planner reproduces, row for row, the tile / split-K / colsum
decisions of the commit before it existed (tests/golden/
gemm_plan_parent.npz, generated from that commit's selection code), and
keeps the invariant the pooled conv forward relies on. Pure host code:
runs without a GPU.

Rows of the dense table are the grid M x N x K x (ta, tb) below in
itertools.product order, plus EXTRA_DENSE; conv rows are conv_shapes()
in order. Paths are stored as indices into PATHS; thin rows record
bm = bn = 0, S = 1, kslice = K.
"""
import itertools
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).parent / "golden" / "gemm_plan_parent.npz"
PATHS = ["none", "thin", "gemm8p", "gemm256", "small"]
ENTRIES = ["fwd", "fwd_pool", "dgrad", "wgrad"]

MS = [1, 7, 47, 48, 49, 96, 97, 108, 512, 720, 4096, 4097, 5904, 8192,
      12544, 32767, 32768, 65535, 65536, 65856, 200704, 802816]
NS = [2, 8, 10, 16, 24, 32, 40, 62, 64, 72, 128, 144, 192, 256, 288, 512,
      576, 1000, 2048]
KS = [5, 8, 16, 24, 32, 40, 64, 72, 144, 288, 576, 1152, 3136, 4608, 25088]
TT = [(False, False), (False, True), (True, False), (True, True)]
# (M, N, K, ta, tb) outside the grid: the gemm8p cases of
# test_gemm_dispatch_gpu.py and its neighbours
EXTRA_DENSE = [(m, m, 512, False, True) for m in (256, 2048, 3328, 3584)]


def dense_rows():
    rows = [(m, n, k, ta, tb) for m, n, k, (ta, tb)
            in itertools.product(MS, NS, KS, TT)]
    return rows + EXTRA_DENSE


def resnet_convs(variant, batch, hw):
    """(N, H, W, C, Kout, R, stride, pad) of every conv of the model in
    bflc_amd/models/resnet.py, in forward order, duplicates dropped."""
    out = []
    if variant == "resnet50":
        out.append((batch, hw, hw, 3, 64, 7, 2, 3))
        hw = (hw + 6 - 7) // 2 + 1
        hw = (hw - 3) // 2 + 1  # 3x3/2 maxpool
        blocks, chans, exp, cin = [3, 4, 6, 3], [64, 128, 256, 512], 4, 64
    else:
        out.append((batch, hw, hw, 3, 16, 3, 1, 1))
        blocks, chans, exp, cin = [3, 3, 3], [16, 32, 64], 1, 16
    for si, (nb, ch) in enumerate(zip(blocks, chans)):
        for bi in range(nb):
            stride = 2 if (bi == 0 and si > 0) else 1
            ohw = (hw + 2 - 3) // stride + 1
            if exp == 4:
                out.append((batch, hw, hw, cin, ch, 1, 1, 0))
                out.append((batch, hw, hw, ch, ch, 3, stride, 1))
                out.append((batch, ohw, ohw, ch, ch * 4, 1, 1, 0))
            else:
                out.append((batch, hw, hw, cin, ch, 3, stride, 1))
                out.append((batch, ohw, ohw, ch, ch, 3, 1, 1))
            if bi == 0 and cin != ch * exp:
                out.append((batch, hw, hw, cin, ch * exp, 1, stride, 0))
            cin, hw = ch * exp, ohw
    return list(dict.fromkeys(out))


def conv_shapes():
    """(N, H, W, C, Kout, R, stride, pad), R x R kernels: every conv
    shape of the GPU conv tests, FEMNIST CNN (batch 32 and 96) and
    ResNet-20 / ResNet-50 (batch 32; 32 and 64 pixel inputs)."""
    s = []
    # test_conv_pool_fused_gpu.py / test_conv_pool_train_gpu.py
    s += [(n, h, w, c, k, 3, 1, 1) for n, h, w, c, k in [
        (8, 8, 8, 32, 64), (3, 6, 6, 32, 64), (5, 12, 12, 32, 64),
        (8, 8, 8, 8, 64), (8, 8, 8, 64, 64), (8, 8, 8, 32, 128),
        (8, 4, 4, 32, 64), (41, 12, 12, 32, 64)]]
    s += [(84, 28, 28, 1, 32, 3, 1, 1), (97, 28, 28, 1, 32, 3, 1, 0),
          (4, 7, 7, 32, 64, 3, 1, 1), (16, 28, 28, 1, 32, 3, 1, 1),
          (4, 10, 10, 32, 64, 3, 2, 1)]
    s += [(n, h, h, 1, k, 3, 1, p) for n, h, k, p in [
        (3, 28, 32, 1), (2, 28, 32, 0), (5, 6, 8, 1), (2, 28, 64, 1)]]
    # test_ops_gpu.py / test_resnet_gpu.py
    s += [(n, h, h, c, k, r, st, p) for n, c, h, k, r, st, p in [
        (4, 1, 28, 32, 3, 1, 1), (4, 32, 14, 64, 3, 1, 1),
        (2, 3, 32, 16, 3, 1, 1), (2, 16, 32, 32, 3, 2, 1),
        (2, 8, 9, 8, 3, 1, 0), (2, 8, 8, 16, 1, 1, 0),
        (2, 3, 32, 16, 7, 2, 3), (96, 1, 28, 32, 3, 1, 1),
        (96, 3, 32, 16, 3, 1, 1), (512, 1, 28, 32, 3, 2, 1),
        (128, 1, 28, 32, 3, 1, 0), (2, 64, 8, 64, 1, 1, 0),
        (2, 16, 16, 32, 3, 2, 1), (2, 64, 14, 256, 1, 1, 0)]]
    # test_gemm_dispatch_gpu.py
    s += [(4, 8, 8, 16, 16, 3, 1, 1)]
    # models
    for b in (32, 96):
        s += [(b, 28, 28, 1, 32, 3, 1, 1), (b, 14, 14, 32, 64, 3, 1, 1)]
    s += resnet_convs("resnet20", 32, 32)
    s += resnet_convs("resnet50", 32, 32) + resnet_convs("resnet50", 32, 64)
    return list(dict.fromkeys(s))


COLSUM_NS = NS + [4, 12, 4096]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


@pytest.fixture(scope="module")
def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def test_dense_table(golden, hip):
    rows = dense_rows()
    want = np.stack([golden["dense_" + f].astype(np.int64)
                     for f in ("path", "bm", "bn", "S", "kslice")], axis=1)
    assert len(rows) == len(want)
    got = np.empty_like(want)
    for i, (m, n, k, ta, tb) in enumerate(rows):
        path, bm, bn, s, kslice = hip.gemm_plan_route(m, n, k, ta, tb)
        got[i] = (PATHS.index(path), bm, bn, s, kslice)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(rows[i], got[i], want[i]) for i in bad[:5]]
    # the table exercises every path and both sides of the wgrad gate
    assert set(want[:, 0]) == {1, 2, 3, 4}
    gate = [480 * (m + n) > m * n for m, n, _, ta, tb in rows
            if ta and not tb]
    assert any(gate) and not all(gate)


def test_conv_table(golden, hip):
    shapes = conv_shapes()
    want = golden["conv"].astype(np.int64)  # [shape][entry][5]
    assert want.shape == (len(shapes), len(ENTRIES), 5)
    for i, (n, h, w, c, kout, r, stride, pad) in enumerate(shapes):
        plans = {}
        for j, e in enumerate(ENTRIES):
            path, *rest = hip.conv_plan_route(e, [n, h, w, c],
                                              [kout, r, r, c], stride, pad)
            plans[e] = (PATHS.index(path), *rest)
            assert plans[e] == tuple(want[i, j]), (shapes[i], e)
        # what keeps conv + pool bitwise: the pooled forward, wherever it
        # applies, runs the plain forward's tile and K slices
        if plans["fwd_pool"][0] != 0:
            assert plans["fwd_pool"] == plans["fwd"], shapes[i]
    assert (want[:, 1, 0] != 0).any() and (want[:, 1, 0] == 0).any()


def test_colsum_table(golden, hip):
    rows = list(itertools.product(MS + [0], COLSUM_NS))
    want = golden["colsum"].astype(np.int64)
    assert want.shape == (len(rows), 4)
    for (m, n), w in zip(rows, want):
        assert hip.colsum_geom(m, n) == tuple(w), (m, n)

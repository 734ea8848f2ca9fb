"""Coverage of the exact GEMM / implicit-conv cases (gemm_exact_cases.py)
and sharpness of their comparison. Pure host code: the route queries
and the fp32 emulation run without a GPU.

The cases must cover every launch-plan class the declared scan grid
reaches, and the reached set must contain the hand-written minimum
below, so shrinking the grid cannot silently shrink coverage. Classes
no case runs are named in EXCLUDED, classes that only explicit extras
run in OUTSIDE_SCAN, each with a reason that test_exclusions checks.
"""
import time

import pytest
import torch

import gemm_exact_cases as gc

SMALL_TILES = [(bm, bn) for bm in (32, 64, 128) for bn in (32, 64, 128)]
DBUF_TILES = [(bm, bn) for bm in (64, 128, 256) for bn in (64, 128, 256)]

def is_dense(k):
    return isinstance(k, gc.DenseKey)


# Classes NO case runs: name -> (predicate on a class key, reason).
# test_exclusions asserts that no reached key and no case matches one.
EXCLUDED = {
    "gemm256 bn=32 (64x32, 128x32)": (
        lambda k: k.path == "gemm256" and k.bn == 32,
        "BFLC_NARROW_DBUF is a default-off experiment"),
    "dgrad gemm256 bn=256": (
        lambda k: k.entry == "dgrad" and k.bn == 256,
        "no caller passes it at the default gates: conv2d_bwd hands the "
        "implicit dgrad C <= 128 only (dgrad_implicit_max_c), and bn=256 "
        "needs N = C % 256 == 0"),
    "wgrad small bm=128": (
        lambda k: k.entry == "wgrad" and k.bm == 128,
        "no caller passes it at the default gates: conv2d_bwd hands the "
        "implicit wgrad Kout <= 64 only (wgrad_implicit_max_kout), so its "
        "GEMM M stays <= 64 and the issue's seven wgrad tiles are six"),
    # not a field of the class key: the route queries plan plain stores,
    # and no entry point can ask for the other store mode
    "EpStore::kConvNCHW epilogues and reduce": (
        None, "EpStore::kConvNCHW has no caller"),
}

# Classes the SCAN does not reach but explicit extras run: name ->
# (predicate, reason). test_exclusions asserts absent from the scan,
# present among the cases.
OUTSIDE_SCAN = {
    "dense gemm256 256x64": (
        lambda k: is_dense(k) and (k.path, k.bm, k.bn) == ("gemm256", 256, 64),
        "no shape under the cap reaches the class: the tile needs "
        "M*N*4 B past the 256 MB partial budget and the dense "
        "double-buffered gate K >= 32, and 1048640 * 64 * 32 > 2e9"),
    "dense thin": (
        lambda k: is_dense(k) and k.path == "thin",
        "the grid's M stops at 4104 and thin starts at M = 65536 (the "
        "shapes are far under the cap; larger M would only add bulk to "
        "every other class)"),
    "conv fwd gemm256 256x64": (
        lambda k: (k.entry, k.path, k.bm, k.bn) == ("fwd", "gemm256", 256, 64),
        "the grid's images stop at 5 x 16 x 16 and the tile needs more "
        "than 1048576 output pixels at Kout = 64 (under the cap at "
        "K = 8, e.g. 5.4e8)"),
    "conv dgrad gemm256 256x64": (
        lambda k: (k.entry, k.path, k.bm, k.bn) == ("dgrad", "gemm256", 256,
                                                     64),
        "as the forward: more than 1048576 input pixels at C = 64"),
}


@pytest.fixture(scope="module")
def scans():
    t0 = time.perf_counter()
    dense, conv = gc.dense_scan(), gc.conv_scan()
    return dense, conv, time.perf_counter() - t0


def all_cases():
    return (list(gc.dense_cases()) + list(gc.thin_cases())
            + [c for e in ("fwd", "dgrad", "wgrad") for c in gc.conv_cases(e)])


def test_cases_cover_every_reached_class(scans):
    dense, conv, wall = scans
    # enumerate the grid again, independently of the cached selection
    reached = set()
    for m, n, k, ta, tb in gc.dense_grid():
        reached.add(gc.dense_key(m, n, k, ta, tb,
                                 gc.dense_route(m, n, k, ta, tb)))
    for entry, shape in gc.conv_grid():
        reached.add(gc.conv_key(entry, shape, gc.conv_route(entry, shape)))
    assert reached == set(dense) | set(conv)
    cases = all_cases()
    covered = {c.key for c in cases}
    uncovered = sorted(map(tuple, reached - covered), key=repr)
    print(f"\nclasses reached: {len(reached)} ({len(dense)} dense, "
          f"{len(conv)} conv); cases: {len(cases)}; scan wall "
          f"{wall:.2f} s; uncovered: {uncovered}")
    assert uncovered == []
    # every stored key is what the route query gives for the stored shape
    for c in cases:
        if isinstance(c, gc.DenseCase):
            assert c.key == gc.dense_case(*c[:5]).key, c
        else:
            assert c.key == gc.conv_case(c.entry, c.shape).key, c
    # scanned cases respect the cap
    for c in list(dense.values()):
        assert c.m * c.n * c.k <= gc.MNK_CAP
    for c in conv.values():
        m, n, k = gc.conv_dims(c.entry, *c.shape)
        assert m * n * k <= gc.MNK_CAP


def test_dense_minimum(scans):
    dense = set(scans[0])
    have = {(k.path, k.bm, k.bn, k.ta, k.tb, k.split) for k in dense}
    # small kernel: nine tiles x four layouts x unsplit / split
    missing = [(t, tt, sp) for t in SMALL_TILES for tt in gc.TT
               for sp in (False, True)
               if ("small", *t, *tt, sp) not in have]
    assert missing == []
    # double-buffered kernel: eight tiles in the scan, each with an M
    # edge and each with a K tail
    for bm, bn in DBUF_TILES:
        if (bm, bn) == (256, 64):
            continue
        ks = [k for k in dense if (k.path, k.bm, k.bn) == ("gemm256", bm, bn)]
        assert any(k.m_edge for k in ks), (bm, bn)
        assert any(k.k_tail for k in ks), (bm, bn)
        assert any(k.m_edge and k.k_tail for k in ks), (bm, bn)
    # ... split wherever the scan finds a split plan of that tile (the
    # list is pinned, so a split plan cannot drop out unnoticed)
    split_tiles = sorted({(k.bm, k.bn) for k in dense
                          if k.path == "gemm256" and k.split})
    assert split_tiles == DBUF_SPLIT_TILES, split_tiles
    # transposed operands with ragged dimensions reach transpose_bf16's
    # edge code: A stored [K, M] with M % 64 and K % 64 != 0, B stored
    # [K, N] with K % 64 != 0
    cases = gc.dense_cases()
    assert any(c.key.path == "gemm256" and c.ta and c.m % 64 and c.k % 64
               for c in cases)
    assert any(c.key.path == "gemm256" and not c.tb and c.k % 64
               for c in cases)
    # both staging forms of the small kernel, on both operands
    vecs = {k.vec for k in dense if k.path == "small"}
    assert vecs == {(a, b) for a in (False, True) for b in (False, True)}
    # both reduce kernels, the tree in all three depths
    assert {k.reduce for k in dense} >= {None, "vec", "tree<=8", "tree9-32",
                                         "tree>32"}
    # whole-K-is-tail under both K steps
    assert any(k.path == "small" and k.k_tail == 2 for k in dense)
    assert any(k.path == "gemm256" and k.k_tail == 2 for k in dense)


# tiles of the double-buffered kernel for which the scan finds S > 1
DBUF_SPLIT_TILES = [(64, 64), (64, 128), (64, 256), (128, 64), (128, 128),
                    (128, 256), (256, 128), (256, 256)]


def test_extras():
    ex = {(c.key.path, c.key.bm, c.key.bn, c.key.split)
          for c in gc.dense_extras()}
    assert ("gemm8p", 256, 256, False) in ex
    assert ("gemm8p", 256, 256, True) in ex
    assert ("gemm256", 256, 64, False) in ex
    by_shape = {c[:3]: c.key for c in gc.dense_extras()}
    k = by_shape[(48, 256, 64)]       # a 256-row tile for 48 rows
    assert (k.path, k.bm, k.m_edge) == ("gemm256", 256, True)
    k = by_shape[(200, 128, 32)]      # K = 32 under a K step of 64
    assert (k.path, k.k_tail) == ("gemm256", 2)
    path, _, _, s, kslice = gc.dense_route(48, 64, 72, False, True)
    assert (path, s, kslice) == ("gemm256", 2, 64)  # second slice 8 deep
    # thin: all four KT at both M, the larger past the 16384-block grid
    thin = gc.thin_cases()
    assert sorted({c.k for c in thin}) == [8, 16, 24, 32]
    assert {c.m for c in thin} == {65536, 16384 * 256 + 257}
    assert len(thin) == 8
    # the thin conv forward is no planner route; its gate is in
    # conv2d_fwd_col: no implicit plan, RSC <= 16, Kout % 8, M >= 65536
    n, h, w, c, kout, r, stride, pad = gc.THIN_CONV
    assert gc.conv_route("fwd", gc.THIN_CONV)[0] == "none"
    assert gc.conv_dims("fwd", *gc.THIN_CONV)[0] > 16384 * 256
    assert r * r * c <= 16 and kout == 8
    # named conv plans
    fwd = {c.shape: c.key for c in gc.conv_cases("fwd")}
    k = fwd[(3, 7, 7, 64, 256, 1, 2, 0)]
    assert (k.path, k.bm, k.m_edge) == ("gemm256", 256, True)
    k = fwd[(3, 8, 8, 8, 64, 1, 2, 0)]
    assert (k.path, k.k_tail) == ("gemm256", 2)
    shape = (3, 4, 4, 64, 8, 3, 1, 1)
    assert shape in {c.shape for c in gc.conv_cases("dgrad")}
    assert gc.conv_route("dgrad", shape)[3:] == (2, 64)
    wg = {c.shape for c in gc.conv_cases("wgrad")}
    for shape, k in [((1, 4, 4, 8, 32, 3, 2, 0), 1),
                     ((1, 4, 4, 128, 32, 1, 2, 0), 4)]:
        assert shape in wg and gc.conv_dims("wgrad", *shape)[2] == k


def test_conv_minimum(scans):
    conv = set(scans[1])
    for entry in ("fwd", "dgrad"):
        have = {(k.path, k.bm, k.bn) for k in conv if k.entry == entry}
        want = [("small", *t) for t in SMALL_TILES]
        want += [("gemm256", bm, 64) for bm in (64, 128)]
        want += [("gemm256", bm, 128) for bm in (64, 128, 256)]
        if entry == "fwd":  # dgrad: see EXCLUDED
            want += [("gemm256", bm, 256) for bm in (64, 128, 256)]
        assert [w for w in want if w not in have] == [], entry
        assert {k.split for k in conv if k.entry == entry} == {False, True}
        # 256x64 comes through the explicit extras, like the dense one,
        # with K shorter than a K step and with a full K step
        tails = {c.key.k_tail for c in gc.conv_cases(entry)
                 if (c.key.path, c.key.bm, c.key.bn) == ("gemm256", 256, 64)}
        assert tails == {1, 2}, (entry, tails)
    have = {(k.path, k.bm, k.bn) for k in conv if k.entry == "wgrad"}
    assert have == {("small", bm, bn) for bm in (32, 64)
                    for bn in (32, 64, 128)}
    assert {k.reduce for k in conv} >= {None, "vec", "tree<=8", "tree9-32",
                                        "tree>32"}


def test_exclusions(scans):
    """The stated exclusions are facts about the reached set: an
    excluded class occurs nowhere, a class outside the scan occurs in
    no scanned key but in some case."""
    dense, conv, _ = scans
    reached = set(dense) | set(conv)
    covered = {c.key for c in all_cases()}
    for name, (pred, reason) in EXCLUDED.items():
        assert reason
        if pred is not None:
            assert [k for k in reached | covered if pred(k)] == [], name
    for name, (pred, reason) in OUTSIDE_SCAN.items():
        assert reason
        assert [k for k in reached if pred(k)] == [], name
        assert any(pred(k) for k in covered), name
    # and every tile of either dispatch table is run, excluded or
    # outside the scan: nothing is left unaccounted for
    run = {(k.entry if not is_dense(k) else "dense", k.path, k.bm, k.bn)
           for k in covered}
    for entry in ("dense", "fwd", "dgrad", "wgrad"):
        want = [("small", *t) for t in SMALL_TILES]
        if entry != "wgrad":
            want += [("gemm256", *t) for t in DBUF_TILES]
        missing = [(entry, *w) for w in want if (entry, *w) not in run]
        named = [m for m in missing
                 if any(p is not None and p(gc.ConvKey(m[0], m[1], m[2], m[3],
                                                      False, False, False, 0,
                                                      None))
                        for p, _ in EXCLUDED.values())]
        unnamed = [m for m in missing if m not in named]
        assert unnamed == [], unnamed


def test_bound_and_amplitudes():
    assert gc.pick_amps(1040) == (127, 127)
    assert gc.pick_amps(1041) == (127, 15)
    assert gc.pick_amps(8806) == (127, 15)
    assert gc.pick_amps(8807) == (15, 15)
    for k in (1, 72, 1040, 4480, 8192, 32768, 10 ** 6):
        for bias in (0, gc.BIAS_UNITS):
            a, b = gc.pick_amps(k, bias)
            assert a * b * k + bias < 1 << 24
    with pytest.raises(AssertionError):
        gc.assert_bound(127, 127, 1041)
    with pytest.raises(AssertionError):
        gc.assert_bound(127, 127, 1040, gc.BIAS_UNITS)
    # operands are exact in bf16 and asymmetric
    a = gc.ints((64, 64), 127, 1, gc.SCALE_A)
    b = gc.ints((64, 64), 127, 2, gc.SCALE_A)
    assert a.dtype == torch.bfloat16 and not torch.equal(a, b)
    assert not torch.equal(a, a.t())
    assert float(a.float().abs().max()) == 127 * gc.SCALE_A


def test_zero_sums_are_plus_zero():
    """A kernel accumulates onto +0, so 0 * negative at K = 1 stores +0;
    the oracle follows that convention, and the comparison still tells
    the two zeros apart."""
    a = torch.tensor([[0.0], [1.0]], dtype=torch.bfloat16)
    b = torch.tensor([[-1.0, 1.0]], dtype=torch.bfloat16)
    want = gc.matmul_oracle(a, b, False, False)
    assert want.view(torch.int16).tolist() == [[0, 0], [-16512, 16256]]
    assert gc.mismatches(-torch.zeros(2, 2, dtype=torch.bfloat16),
                         torch.zeros(2, 2, dtype=torch.bfloat16)) == 4
    # the smallest cases of the scan are K = 1: none expects a -0
    n = 0
    for c in gc.dense_cases():
        if c.k == 1 and c.m * c.n <= 1024:
            amp_a, amp_b = gc.pick_amps(1)
            x = gc.ints((c.m, 1), amp_a, 1, gc.SCALE_A)
            y = gc.ints((1, c.n), amp_b, 2, gc.SCALE_B)
            want = gc.matmul_oracle(x, y, False, False)
            assert int((want.view(torch.int16) == -32768).sum()) == 0
            n += 1
    assert n > 0


def emulate(a, b, order=1):
    """fp32 GEMM in K blocks of 32, summed ascending or descending."""
    m, k = a.shape
    acc = torch.zeros(m, b.shape[1], dtype=torch.float32)
    for k0 in list(range(0, k, 32))[::order]:
        acc = acc + a[:, k0:k0 + 32].float() @ b[k0:k0 + 32].float()
    return acc


@pytest.mark.parametrize("k", [72, 1040, 8192])
def test_comparison_is_sharp(k):
    """Against an fp32 emulation of a GEMM: the right result matches
    the oracle bit for bit in either summation order, and each of four
    plausible kernel mistakes does not."""
    m = n = 96  # square, so a transposed output has the right shape
    amp_a, amp_b = gc.pick_amps(k)
    a = gc.ints((m, k), amp_a, 1, gc.SCALE_A)
    b = gc.ints((k, n), amp_b, 2, gc.SCALE_B)
    want = gc.matmul_oracle(a, b, False, False)
    good = emulate(a, b)
    assert gc.mismatches(good.bfloat16(), want) == 0
    assert gc.mismatches(emulate(a, b, -1).bfloat16(), want) == 0
    assert torch.equal(good, emulate(a, b, -1))  # exact, not just close

    def bad(x):
        return gc.mismatches(x.bfloat16(), want)

    assert bad(emulate(a[:, :-1], b[:-1])) > 0       # last K element dropped
    k0 = (k // 32 - 1) * 32                          # one K step twice
    assert bad(good + a[:, k0:k0 + 32].float() @ b[k0:k0 + 32].float()) > 0
    assert bad(good.t().contiguous()) > 0            # output transposed
    unwritten = good.clone()
    unwritten[-1] = 0                                # last row unwritten
    assert bad(unwritten) > 0
    # the four layouts of the oracle agree with each other
    for ta, tb in gc.TT:
        aa = a.t().contiguous() if ta else a
        bb = b.t().contiguous() if tb else b
        assert gc.mismatches(gc.matmul_oracle(aa, bb, ta, tb), want) == 0


def test_conv_oracles_agree_with_matmul():
    """The conv oracles against the matmul oracle on a hand-built im2col
    (1x1 stride 2: the gather is a strided slice), so a layout slip in
    the oracle itself cannot hide."""
    n, h, c, kout = 2, 5, 8, 16
    x = gc.ints((n, h, h, c), 127, 1, gc.SCALE_A)
    w = gc.ints((kout, 1, 1, c), 127, 2, gc.SCALE_B)
    y = gc.conv_fwd_oracle(x, w, 2, 0)
    col = x[:, ::2, ::2, :].reshape(-1, c).contiguous()
    want = gc.matmul_oracle(col, w.reshape(kout, c), False, True)
    assert gc.mismatches(y.reshape(-1, kout), want) == 0
    dy = gc.ints(tuple(y.shape), 127, 3, gc.SCALE_DY)
    dx = gc.conv_bwd_oracle(x, w, dy, 2, 0, 0)
    dw = gc.conv_bwd_oracle(x, w, dy, 2, 0, 1)
    dy2 = dy.reshape(-1, kout)
    want_dw = gc.matmul_oracle(dy2, col, True, False)
    assert gc.mismatches(dw.reshape(kout, c), want_dw) == 0
    want_dx = gc.matmul_oracle(dy2, w.reshape(kout, c), False, False)
    assert gc.mismatches(dx[:, ::2, ::2, :].reshape(-1, c), want_dx) == 0
    assert float(dx[:, 1::2].float().abs().max()) == 0

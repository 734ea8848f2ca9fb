"""Shared pieces of the exact GEMM / implicit-conv tests
(test_gemm_exact_cases.py on the host, test_gemm_exact_gpu.py on the
GPU): inputs whose products sum exactly in fp32, the float64 oracles,
the class key of a launch plan, and the scan that picks one smallest
case per class the planner reaches.

Why no tolerance is needed. Operands are small integers times a power of
two (A: |k| <= ampA at 2^-6, B: |k| <= ampB at 2^-10), so every product
is a multiple of one unit (2^-16) and, while

    ampA * ampB * K + |bias in units| < 2^24,

every partial sum taken in ANY order is an integer number of units below
2^24: exact in fp32. MFMA accumulation, split-K partials, both reduce
trees and the bias add therefore round nowhere, the kernel's only
rounding is the final fp32 -> bf16 store, and the expected output is
the float64 result rounded once, which the kernel must equal bitwise.
assert_bound() checks that condition for every case; it is a
precondition of the method, not a measurement.

Nothing here needs a GPU: the route queries are pure host code.
"""
import functools
import itertools
from collections import namedtuple

import torch
import torch.nn.functional as F

TT = [(False, False), (False, True), (True, False), (True, True)]

BOUND = 1 << 24
# operand scales (powers of two; every |k| <= 127 is exact in bf16)
SCALE_A = 2.0 ** -6
SCALE_B = 2.0 ** -10
SCALE_DY = 2.0 ** -8    # conv backward's upstream gradient
# bias = kb * 2^-10, |kb| <= BIAS_AMP: kb * 64 units of 2^-16
SCALE_BIAS = 2.0 ** -10
BIAS_AMP = 127
BIAS_UNITS = BIAS_AMP * 64

# (ampA, ampB) rungs, widest first: 127 x 127 serves K <= 1040 and
# 127 x 15 serves K <= 8806 (bias-free); deeper K shrinks further.
AMP_LADDER = [(127, 127), (127, 15), (15, 15), (15, 3), (3, 3), (3, 1),
              (1, 1)]


def assert_bound(amp_a, amp_b, k, bias_units=0):
    """Every partial sum of K products (plus the bias) stays an integer
    number of units below 2^24, i.e. exact in fp32 in any order."""
    worst = amp_a * amp_b * k + bias_units
    assert worst < BOUND, (amp_a, amp_b, k, bias_units, worst)


def pick_amps(k, bias_units=0):
    """The widest amplitude pair the bound allows at this K."""
    for a, b in AMP_LADDER:
        if a * b * k + bias_units < BOUND:
            assert_bound(a, b, k, bias_units)
            return a, b
    raise AssertionError(f"K = {k} is too deep for an exact fp32 sum")


def ints(shape, amp, seed, scale):
    """bf16 tensor of k * scale, k uniform in [-amp, amp] from a seeded
    CPU generator (a different seed per operand keeps them asymmetric)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-amp, amp + 1, tuple(shape), generator=g,
                      dtype=torch.int16)
    return (k.to(torch.float32) * scale).to(torch.bfloat16)


def round_once(acc64, bias=None, relu=False):
    """float64 accumulator -> the kernel's epilogue: + bias, ReLU, one
    rounding to bf16. Also checks what the bound promises: the value
    before that rounding is exactly an fp32 number.

    The kernels add every product onto a +0 accumulator, so a sum that
    is exactly zero is +0 whatever the signs of its terms ((-0) + (+0)
    = +0, x + (-x) = +0 in round-to-nearest). A float64 matmul at K = 1
    returns the bare product instead, -0 for 0 * negative; adding +0
    puts that one convention back, and the comparison stays bitwise."""
    acc64 = acc64 + 0.0
    if bias is not None:
        acc64 = acc64 + bias.double()
    if relu:
        acc64 = acc64.clamp_min(0)
    f = acc64.float()
    assert torch.equal(f.double(), acc64), "oracle not exact in fp32"
    return f.bfloat16()


def matmul_oracle(a, b, ta, tb, bias=None, relu=False):
    """op(a) @ op(b) for the four (ta, tb) storage layouts of gemm_raw:
    ta: a is stored [K, M]; tb: b is stored [N, K]."""
    a64 = a.double().t() if ta else a.double()
    b64 = b.double().t() if tb else b.double()
    return round_once(a64 @ b64, bias, relu)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def conv_fwd_acc(x, w, stride, pad):
    """NHWC x [N,H,W,C], KRSC w [Kout,R,S,C] -> NHWC float64 accumulator
    of F.conv2d."""
    y = F.conv2d(_nchw(x), _nchw(w), None, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_fwd_oracle(x, w, stride, pad, bias=None, relu=False):
    return round_once(conv_fwd_acc(x, w, stride, pad), bias, relu)


def conv_bwd_oracle(x, w, dy, stride, pad, which):
    """dx (NHWC, which = 0) or dw (KRSC, which = 1): the autograd
    gradient of the float64 F.conv2d."""
    ops = [_nchw(x).contiguous(), _nchw(w).contiguous()]
    ops[which].requires_grad_()
    y = F.conv2d(ops[0], ops[1], None, stride, pad)
    g, = torch.autograd.grad(y, ops[which], _nchw(dy).contiguous())
    return round_once(g.permute(0, 2, 3, 1).contiguous())


def mismatches(got, want):
    """Number of elements whose bit patterns differ; shape and dtype
    must agree outright."""
    assert got.dtype == want.dtype == torch.bfloat16, (got.dtype, want.dtype)
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return int((got.contiguous().view(torch.int16)
                != want.contiguous().view(torch.int16)).sum())


# ---------------------------------------------------------------------------
# class keys
# ---------------------------------------------------------------------------

K_STEP = {"small": 32, "gemm256": 64, "gemm8p": 64}


def k_tail(k, step):
    """0: K is whole K steps; 1: a partial last step; 2: K is shorter
    than one step, so the whole K extent is tail."""
    return 0 if k % step == 0 else (2 if k < step else 1)


def reduce_kind(m, n, s):
    """Which split-K reduce runs (launch_splitk_reduce): the float4
    serial walk, or the 8-lane tree by how far its 32-stride loop gets."""
    if s <= 1:
        return None
    if n % 4 == 0 and m * n >= 131072:
        return "vec"
    return "tree<=8" if s <= 8 else ("tree9-32" if s <= 32 else "tree>32")


DenseKey = namedtuple(
    "DenseKey", "entry ta tb path bm bn split m_edge n_edge k_tail vec reduce")
ConvKey = namedtuple(
    "ConvKey", "entry path bm bn split m_edge n_edge k_tail reduce")


def dense_key(m, n, k, ta, tb, route):
    path, bm, bn, s, _ = route
    if path == "thin":  # one kernel per KT = K and no tile: the k_tail
        # field carries KT
        return DenseKey("dense", ta, tb, path, 0, 0, False, False, False,
                        k, None, None)
    vec = None
    if path == "small":  # the launcher's 16-B staging flags
        vec = (m % 8 == 0 if ta else k % 8 == 0,
               k % 8 == 0 if tb else n % 8 == 0)
    return DenseKey("dense", ta, tb, path, bm, bn, s > 1, m % bm != 0,
                    n % bn != 0, k_tail(k, K_STEP[path]), vec,
                    reduce_kind(m, n, s))


def conv_dims(entry, n, h, w, c, kout, r, stride, pad):
    """(M, N, K) of the entry's GEMM view (conv_gemm_dims)."""
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w + 2 * pad - r) // stride + 1
    if entry == "wgrad":
        return kout, r * r * c, n * oh * ow
    if entry == "dgrad":
        return n * h * w, c, r * r * kout
    return n * oh * ow, kout, r * r * c


def conv_key(entry, shape, route):
    path, bm, bn, s, _ = route
    m, n, k = conv_dims(entry, *shape)
    return ConvKey(entry, path, bm, bn, s > 1, m % bm != 0, n % bn != 0,
                   k_tail(k, K_STEP[path]), reduce_kind(m, n, s))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

DenseCase = namedtuple("DenseCase", "m n k ta tb key")
# shape = (n, h, w, c, kout, r, stride, pad), r x r kernels
ConvCase = namedtuple("ConvCase", "entry shape key")

MNK_CAP = 2 * 10 ** 9  # no scanned case is larger than this M*N*K

# The declared scan grid of the dense entry. M: both sides of the 48 /
# 96 tile thresholds and of the M >= 48 double-buffered gate, rows that
# are no multiple of 8 or of a tile, and > 4096 (pick_tile's shrink).
DENSE_MS = [1, 8, 33, 40, 47, 48, 49, 64, 96, 97, 100, 128, 200, 256, 264,
            512, 520, 1024, 4104]
DENSE_NS = [8, 10, 24, 32, 40, 62, 64, 72, 100, 128, 136, 192, 256, 320, 512]
DENSE_KS = [1, 5, 8, 24, 32, 40, 64, 72, 100, 128, 200, 520, 1040, 2048,
            4104, 8192]

# Plans named one by one: (m, n, k, ta, tb, (path, bm, bn, split)).
DENSE_EXTRAS = [
    # gemm8p, unsplit and split
    (3584, 3584, 64, False, True, ("gemm8p", 256, 256, False)),
    (1536, 2048, 4480, False, True, ("gemm8p", 256, 256, True)),
    # ... and in linear_fwd's layout, for its bias / ReLU epilogues
    (3584, 3584, 64, False, False, ("gemm8p", 256, 256, False)),
    (1536, 2048, 4480, False, False, ("gemm8p", 256, 256, True)),
    # 256x64: only past pick_splitk's 256 MB partial budget (M*N*4 B)
    (1048640, 64, 32, False, False, ("gemm256", 256, 64, False)),
    # a 256-row double-buffered tile for M = 48
    (48, 256, 64, False, True, None),
    # the double-buffered kernel with its whole K extent one tail
    (200, 128, 32, False, True, None),
    # S = 2 with kslice = 64 on K = 72: the second slice is 8 deep
    (48, 64, 72, False, True, None),
]
THIN_KS = [8, 16, 24, 32]
# the thin kernels' grid is capped at 16384 blocks of 256 rows: the
# second M walks the grid-stride loop, with a ragged last block
THIN_MS = [65536, 16384 * 256 + 257]
THIN_N = 8

CONV_NS = [1, 2, 3, 5]
CONV_HWS = [4, 7, 8, 12, 16]
# 40 and 72: N above 32 / 64 that is no multiple of 64 keeps the small
# kernel, at its 64- and 128-wide tiles (N = Kout forward, N = C dgrad)
CONV_CS = [8, 16, 24, 32, 40, 64, 72, 128, 256]
CONV_KOUTS = [8, 16, 24, 32, 40, 64, 72, 128, 256]
CONV_RSP = [(1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 2, 0), (5, 1, 2)]

# Plans named one by one: (entry, shape, (path, bm, bn, S) or None).
CONV_EXTRAS = [
    # 256-row tile for M = 48
    ("fwd", (3, 7, 7, 64, 256, 1, 2, 0), ("gemm256", 256, 256, 1)),
    # K = 8 under a K step of 64
    ("fwd", (3, 8, 8, 8, 64, 1, 2, 0), None),
    # S = 2 with kslice = 64 on K = 72: the second slice is 8 deep
    ("dgrad", (3, 4, 4, 64, 8, 3, 1, 1), ("gemm256", 128, 64, 2)),
    ("wgrad", (1, 4, 4, 8, 32, 3, 2, 0), None),    # GEMM K = 1
    ("wgrad", (1, 4, 4, 128, 32, 1, 2, 0), None),  # GEMM K = 4
    # 256x64: M * 64 * 4 B past the 256 MB partial budget, as in the dense
    # entry, but an implicit conv gets there with a shallow K and far
    # below the cap; the grid's images are just too small (M <= 1280).
    # Forward with K = 8 (all tail) and K = 72 (a full K step first: the
    # guard-free staging of interior tiles), dgrad likewise.
    ("fwd", (5, 458, 458, 8, 64, 1, 1, 1), ("gemm256", 256, 64, 1)),
    ("fwd", (5, 460, 460, 8, 64, 3, 1, 1), ("gemm256", 256, 64, 1)),
    ("dgrad", (5, 460, 460, 64, 8, 1, 1, 1), ("gemm256", 256, 64, 1)),
    ("dgrad", (5, 460, 460, 64, 8, 3, 1, 1), ("gemm256", 256, 64, 1)),
]
# thin conv forward (C = 1, 3x3: KT = 16) with more than 16384 * 256
# output pixels at Kout = 8: (n, h, w, c, kout, r, stride, pad)
THIN_CONV = (17, 500, 500, 1, 8, 3, 1, 1)


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def dense_route(m, n, k, ta, tb):
    return hip().gemm_plan_route(m, n, k, ta, tb)


def conv_route(entry, shape):
    n, h, w, c, kout, r, stride, pad = shape
    return hip().conv_plan_route(entry, [n, h, w, c], [kout, r, r, c],
                                 stride, pad)


def conv_entry_taken(entry, shape):
    """Whether conv2d_fwd / conv2d_bwd really hand this shape to the
    implicit entry: the gates of csrc/hip/conv2d.hip that sit in front
    of the planner. 1x1 stride-1 convs are dense GEMMs on a view of x;
    the implicit dgrad serves stride 1 and 8 <= C <= 128, the implicit
    wgrad Kout <= 64. Everything else takes the dcol + col2im or
    materialized-col fallbacks, which are no subject of these tests.

    Limitation: this is a copy of those gates (at their defaults; both
    are environment-overridable there), because conv2d.hip exports no
    route query for conv2d_bwd or for the thin conv forward. If the
    dgrad gate moved, the dcol + col2im fallback would show: it rounds
    twice and cannot match a once-rounded oracle. If the wgrad gate or
    the thin conv gate moved, the materialized-col GEMM is once-rounded
    too, so the 'wgrad' and thin-conv cases would still pass while
    running a dense kernel under an implicit class label. The copy has
    to be kept in step by hand until such a query exists."""
    n, h, w, c, kout, r, stride, pad = shape
    if r == 1 and stride == 1 and pad == 0:
        return False
    if h + 2 * pad < r:
        return False
    if entry == "dgrad" and not (kout % 8 == 0 and 8 <= c <= 128
                                 and stride == 1):
        return False
    if entry == "wgrad" and kout > 64:
        return False
    return conv_route(entry, shape)[0] != "none"


def dense_grid():
    for m, n, k in itertools.product(DENSE_MS, DENSE_NS, DENSE_KS):
        if m * n * k <= MNK_CAP:
            for ta, tb in TT:
                yield m, n, k, ta, tb


def conv_grid():
    for entry in ("fwd", "dgrad", "wgrad"):
        for n, hw, c, kout, (r, stride, pad) in itertools.product(
                CONV_NS, CONV_HWS, CONV_CS, CONV_KOUTS, CONV_RSP):
            shape = (n, hw, hw, c, kout, r, stride, pad)
            if conv_entry_taken(entry, shape):
                m, nn, k = conv_dims(entry, *shape)
                if m * nn * k <= MNK_CAP:
                    yield entry, shape


def _keep_smallest(best, key, size, case):
    if key not in best or size < best[key][0]:
        best[key] = (size, case)


@functools.lru_cache(maxsize=None)
def dense_scan():
    """{class key: smallest-M*N*K DenseCase} over the dense grid."""
    best = {}
    for m, n, k, ta, tb in dense_grid():
        key = dense_key(m, n, k, ta, tb, dense_route(m, n, k, ta, tb))
        _keep_smallest(best, key, m * n * k, DenseCase(m, n, k, ta, tb, key))
    return {key: case for key, (_, case) in best.items()}


@functools.lru_cache(maxsize=None)
def conv_scan():
    """{class key: smallest-M*N*K ConvCase} over the conv grid."""
    best = {}
    for entry, shape in conv_grid():
        key = conv_key(entry, shape, conv_route(entry, shape))
        m, n, k = conv_dims(entry, *shape)
        _keep_smallest(best, key, m * n * k, ConvCase(entry, shape, key))
    return {key: case for key, (_, case) in best.items()}


def dense_case(m, n, k, ta, tb):
    return DenseCase(m, n, k, ta, tb,
                     dense_key(m, n, k, ta, tb, dense_route(m, n, k, ta, tb)))


def conv_case(entry, shape):
    assert conv_entry_taken(entry, shape), (entry, shape)
    return ConvCase(entry, shape,
                    conv_key(entry, shape, conv_route(entry, shape)))


@functools.lru_cache(maxsize=None)
def dense_extras():
    out = []
    for m, n, k, ta, tb, want in DENSE_EXTRAS:
        case = dense_case(m, n, k, ta, tb)
        if want is not None:  # the plan the extra is listed for
            got = (case.key.path, case.key.bm, case.key.bn, case.key.split)
            assert got == want, (m, n, k, ta, tb, got, want)
        out.append(case)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def thin_cases():
    out = []
    for m, k in itertools.product(THIN_MS, THIN_KS):
        case = dense_case(m, THIN_N, k, False, True)
        assert case.key.path == "thin" and case.key.k_tail == k, case
        out.append(case)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dense_cases():
    """Scan picks + extras, thin cases apart (thin_cases())."""
    picked = [c for c in dense_scan().values() if c.key.path != "thin"]
    seen = {c[:5] for c in picked}
    extra = [c for c in dense_extras() if c[:5] not in seen]
    return tuple(sorted(picked + extra, key=lambda c: (c.m * c.n * c.k, c)))


@functools.lru_cache(maxsize=None)
def conv_cases(entry):
    picked = [c for c in conv_scan().values() if c.entry == entry]
    seen = {c.shape for c in picked}
    extra = []
    for e, s, want in CONV_EXTRAS:
        if e != entry:
            continue
        if want is not None:  # the plan the extra is listed for
            assert conv_route(e, s)[:4] == want, (e, s, conv_route(e, s))
        if s not in seen:
            extra.append(conv_case(e, s))
    return tuple(sorted(picked + extra, key=lambda c: c.shape))


def linear_fwd_cases():
    """Non-transposed dense cases, the smallest per (path, tile, split,
    reduce kernel): what linear_fwd adds to gemm_raw is the bias / ReLU
    epilogue of each kernel and of each reduce."""
    best = {}
    for c in dense_cases():
        if c.ta or c.tb:
            continue
        k = (c.key.path, c.key.bm, c.key.bn, c.key.split, c.key.reduce)
        _keep_smallest(best, k, c.m * c.n * c.k, c)
    return tuple(case for _, case in best.values())


# (M, K, N) of x [M, K] @ w [K, N], then the plans (path, bm, bn, S) of
# linear_bwd's two GEMMs: dx = dy @ w^T is the (False, True) GEMM
# [M, K] over N, dw = x^T @ dy the (True, False) GEMM [K, N] over M.
# Small and double-buffered tiles, unsplit and split (S up to 65), ragged
# edges, and one dw large enough to leave the routed-small wgrad layout
# for the double-buffered kernel behind two operand transposes.
LINEAR_BWD = [
    ((100, 40, 24), ("small", 128, 64, 1), ("small", 32, 32, 4)),
    ((33, 72, 62), ("small", 32, 128, 2), ("small", 64, 64, 2)),
    ((48, 256, 64), ("gemm256", 256, 256, 1), ("small", 128, 64, 2)),
    ((200, 72, 128), ("small", 128, 128, 4), ("small", 64, 128, 4)),
    ((520, 128, 192), ("gemm256", 128, 128, 2), ("small", 128, 128, 9)),
    ((64, 4104, 128), ("small", 64, 128, 4), ("small", 32, 128, 1)),
    ((4104, 64, 32), ("gemm256", 64, 64, 1), ("small", 64, 32, 65)),
    ((264, 1040, 320), ("small", 128, 128, 5), ("small", 128, 128, 5)),
    ((256, 1024, 1024), ("gemm256", 64, 256, 8), ("gemm256", 64, 256, 1)),
]


def linear_bwd_routes(m, k, n):
    """(path, bm, bn, S) of the dx and the dw GEMM."""
    return (dense_route(m, k, n, False, True)[:4],
            dense_route(k, n, m, True, False)[:4])

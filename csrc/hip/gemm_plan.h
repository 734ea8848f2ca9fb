// Host-side GEMM planning: which kernel family, tile and split-K slice
// count a shape gets, and the colsum chunk geometry. Pure C++17 (no
// torch, no HIP) so the launchers, the route queries and a plain g++
// test all run the same functions. Every bitwise guarantee between two
// entry points (pooled vs plain conv forward, fused vs two-pass bias
// gradients) rests on both asking the one plan function here.
#pragma once

#include <algorithm>

namespace bflc {

constexpr int kSmallBK = 32;  // K step of gemm_kernel (BK)
constexpr int kDbufBK = 64;   // K step of gemm256_kernel / gemm8p (BK2)

inline long plan_ceil(long a, long b) { return (a + b - 1) / b; }

// Choose the split-K slice count minimizing estimated GEMM + reduce
// time: gemm ~ 2MNK/tf scaled by chip fill (block_target blocks fill
// the 256 CUs at this path's occupancy), reduce ~ (S+1)*M*N*4B at
// ~6 TB/s. Replaces the fixed-target heuristics that either starved
// tiny-output wgrads of occupancy or drowned mid-size outputs in
// partial-buffer traffic.
inline long pick_splitk(long M, long N, long K, long tiles, long ksteps,
                        int block_target, double tf,
                        double* time_out = nullptr) {
  const long budget = (256L << 20) / std::max<long>(M * N * 4, 1);
  const long smax = std::min<long>({ksteps, budget, 512});
  const double work = 2.0 * (double)M * N * K / tf;
  double best_t = 1e30;
  long best_s = 1;
  for (long s = 1; s <= smax; s *= 2) {
    const double fill =
        std::min(1.0, (double)(tiles * s) / block_target);
    // short per-slice K chains never amortize the staging prologue;
    // the measured reduce pass runs ~2.5 TB/s, not peak HBM
    const double steps = (double)ksteps / s;
    const double eff = steps / (steps + 4.0);
    const double t = work / std::max(fill * eff, 1e-3) +
                     (s > 1 ? (s + 1.0) * M * N * 4 / 2.5e12 : 0.0);
    if (t < best_t) { best_t = t; best_s = s; }
  }
  if (time_out) *time_out = best_t;
  return best_s;
}

struct TileCfg { int bm, bn, wr, wc; };

inline TileCfg pick_tile(long M, long N) {
  int bn = N <= 32 ? 32 : (N <= 64 ? 64 : 128);
  int bm = M <= 48 ? 32 : (M <= 96 ? 64 : 128);
  // keep >= ~512 tiles when possible by shrinking BM (conv fwd shapes
  // have huge M, so this rarely triggers; fc shapes are latency-bound
  // anyway)
  auto tiles = [&](int m, int n) {
    return plan_ceil(M, m) * plan_ceil(N, n);
  };
  while (bm > 32 && tiles(bm, bn) < 512 && M > 4096) bm /= 2;
  int wr = bm >= 64 ? 2 : (bm == 32 ? 1 : 2);
  int wc = 2;
  if (bm == 32) { wr = 1; wc = 4; }
  if (bn == 32 && bm == 32) { wr = 2; wc = 1; }
  if (bn == 32 && bm > 32) { wr = 2; wc = 2; }
  return {bm, bn, wr, wc};
}

enum class GemmPath { kNone, kThin, kGemm8p, kGemm256, kSmall };

inline const char* gemm_path_name(GemmPath p) {
  switch (p) {
    case GemmPath::kThin: return "thin";
    case GemmPath::kGemm8p: return "gemm8p";
    case GemmPath::kGemm256: return "gemm256";
    case GemmPath::kSmall: return "small";
    default: return "none";
  }
}

// One launch: grid = (tiles, S), each slice covers kslice of K. wr/wc
// (waves per tile row/column) are set for the small-tile family only;
// the double-buffered kernels always run 8 waves.
struct GemmPlan {
  GemmPath path = GemmPath::kNone;
  int bm = 0, bn = 0, wr = 0, wc = 0;
  long tiles = 0, S = 1, kslice = 0;
};

// Slices are whole K steps; S becomes the count of non-empty slices.
inline void set_slices(GemmPlan& p, long K, long ksteps, long S, int bk) {
  p.kslice = plan_ceil(ksteps, S) * bk;
  p.S = plan_ceil(K, p.kslice);
}

// Synchronous small-tile family (gemm_kernel): split K when the tile
// grid cannot fill the chip and K is deep.
inline GemmPlan plan_small(long M, long N, long K) {
  const TileCfg t = pick_tile(M, N);
  GemmPlan p;
  p.path = GemmPath::kSmall;
  p.bm = t.bm; p.bn = t.bn; p.wr = t.wr; p.wc = t.wc;
  p.tiles = plan_ceil(M, t.bm) * plan_ceil(N, t.bn);
  const long ksteps = plan_ceil(K, kSmallBK);
  set_slices(p, K, ksteps,
             pick_splitk(M, N, K, p.tiles, ksteps, 512, 150.0e12),
             kSmallBK);
  return p;
}

// Rough per-tile efficiency of the double-buffered family from the
// measured ladder (64-tile structures run far below the 256 ones);
// narrow tiles are staging-heavier.
inline double dbuf_tile_tf(int bm) {
  return bm == 256 ? 800.0e12 : (bm == 128 ? 600.0e12 : 320.0e12);
}
constexpr double kDbufBn64Penalty = 0.75;

// Double-buffered BMxBN family (gemm256_kernel; needs N % 64 == 0):
// tile and split-K chosen together by the cost model.
// (a BN=32 config measured slower than the synchronous 128x32 path
// on the shallow-K shapes it would serve; BN=64 stays the floor, and
// N edges are zero-staged + epilogue-guarded like M edges)
inline GemmPlan plan_dbuf(long M, long N, long K) {
  GemmPlan p;
  p.path = GemmPath::kGemm256;
  p.bn = (N % 256 == 0) ? 256 : (N % 128 == 0 ? 128 : 64);
  const long ksteps = plan_ceil(K, kDbufBK);
  const long ntn = plan_ceil(N, p.bn);
  const double bn_pen = p.bn >= 128 ? 1.0 : kDbufBn64Penalty;
  double best_t = 1e30;
  long S = 1;
  // outputs past pick_splitk's 256 MB partial budget get no estimate
  // at all and keep this default (also the only way to 256x64)
  p.bm = 256;
  for (int bm : {256, 128, 64}) {
    if (bm == 256 && p.bn == 64) continue;
    double t;
    const long s = pick_splitk(M, N, K, plan_ceil(M, bm) * ntn, ksteps, 256,
                               dbuf_tile_tf(bm) * bn_pen, &t);
    if (t < best_t) { best_t = t; p.bm = bm; S = s; }
  }
  p.tiles = plan_ceil(M, p.bm) * ntn;
  set_slices(p, K, ksteps, S, kDbufBK);
  return p;
}

// The BN == 32 double-buffered experiment (BFLC_NARROW_DBUF=1; see
// conv_implicit_gemm): tile by M alone, 450 / 250 TF.
inline GemmPlan plan_dbuf_narrow(long M, long N, long K) {
  GemmPlan p;
  p.path = GemmPath::kGemm256;
  p.bm = M >= 32768 ? 128 : 64;
  p.bn = 32;
  p.tiles = plan_ceil(M, p.bm) * plan_ceil(N, 32);
  const long ksteps = plan_ceil(K, kDbufBK);
  set_slices(p, K, ksteps,
             pick_splitk(M, N, K, p.tiles, ksteps, 256,
                         p.bm == 128 ? 450.0e12 : 250.0e12),
             kDbufBK);
  return p;
}

// Dense entry (gemm_bf16_raw). plain_store: EpStore::kPlain;
// want_stats: the caller asked for fused BN partials; wgrad_small: the
// BFLC_WGRAD_SMALL gate (-1 never, 1 always, 0 = the cost gate below).
inline GemmPlan plan_dense(long M, long N, long K, bool ta, bool tb,
                           bool plain_store, bool want_stats,
                           int wgrad_small) {
  // thin memory-shaped GEMMs (conv stems after K padding: FEMNIST
  // conv1 K=16 N=32, CIFAR stems K=32 N=16) bypass the MFMA tilers
  if (!ta && tb && K <= 32 && K % 8 == 0 && N <= 64 && N % 8 == 0 &&
      M >= 65536 && plain_store && !want_stats) {
    GemmPlan p;
    p.path = GemmPath::kThin;
    p.tiles = std::min<long>(plan_ceil(M, 256), 16384);
    p.kslice = K;
    return p;
  }
  // Route wgrad-layout GEMMs (ta, !tb — both operands K-major) straight
  // to the small kernel's swizzled scatter staging when the two operand
  // transposes the dbuf path would need outweigh the GEMM itself:
  // t_transpose ~ 4K(M+N)/5e12 vs t_gemm ~ 2MNK/600e12, i.e. when
  // 480(M+N) > MN (all wgrad outputs qualify; big square GEMMs do not).
  // (A/B on ResNet-50: 81.2 default-off vs 80.7 ms/round routed small.)
  const bool route_small =
      ta && !tb &&
      (wgrad_small == 1 ||
       (wgrad_small == 0 && 480.0 * (double)(M + N) > (double)M * N));
  // N%64 floor: widening to N%8 routed mid shapes onto narrow-BN
  // configs that measured slower than the synchronous path (the edge
  // guards stay for M and the K tail).
  if (!route_small && N % 64 == 0 && K % 8 == 0 && M >= 48 && N >= 64 &&
      K >= 32) {
    GemmPlan p = plan_dbuf(M, N, K);
    // fully aligned large shapes take the 8-phase glds schedule
    // (also at shallow K: an A/B routing K-slices < 8 tiles to the
    // double-buffered kernel measured +9% on a ResNet-50 round)
    if (p.bm == 256 && p.bn == 256 && M % 256 == 0 && N % 256 == 0 &&
        K % 64 == 0 && plain_store)
      p.path = GemmPath::kGemm8p;
    return p;
  }
  return plan_small(M, N, K);
}

// Implicit-GEMM conv entries (fwd / dgrad) on their GEMM view.
// narrow-N convs (ResNet-20's Kout 16/32) run the implicit gather in
// the synchronous small-tile kernel — the col read it replaces is the
// traffic bound there (col is R*S times the activation).
inline GemmPlan plan_conv(long M, long N, long K, bool narrow_dbuf) {
  if (N % 64 == 0 && N >= 64) return plan_dbuf(M, N, K);
  if (narrow_dbuf && N <= 32 && M >= 8192) return plan_dbuf_narrow(M, N, K);
  return plan_small(M, N, K);
}

// Hierarchical colsum of an [M, N] matrix: pass 1 runs cblocks x chunks
// blocks, each reducing `rows` rows of G 16-B column granules (N % 8
// == 0) or of 32 scalar columns — a few waves per SIMD across the 256
// CUs, from the shape alone — and pass 2 reduces the chunks.
struct ColsumGeom { int G, cblocks; long rows; int chunks; };

inline ColsumGeom colsum_geom(long M, long N) {
  ColsumGeom g;
  g.G = 1;
  while (g.G * 2 <= std::min<long>(N / 8, 256)) g.G *= 2;
  g.cblocks = (int)(N % 8 == 0 ? plan_ceil(N / 8, g.G) : plan_ceil(N, 32));
  const long target =
      std::max<long>(1, std::min<long>(768 / std::max(g.cblocks, 1), 256));
  g.rows = std::max<long>(64, plan_ceil(M, target));
  g.chunks = (int)plan_ceil(M, g.rows);
  return g;
}

// float4 column granules per block of the vector final pass (N % 4 ==
// 0); <= 16 so every block keeps >= 16 chunk-lanes.
inline int colsum_final_g4(long N) {
  int g4 = 1;
  while (g4 * 2 <= std::min<long>(N / 4, 16)) g4 *= 2;
  return g4;
}

}  // namespace bflc

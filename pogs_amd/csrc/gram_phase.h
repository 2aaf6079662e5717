#pragma once
// The Gram phase of the dense factorisation: G = P^T P for a K-major operand, by the product the shape calls for
// (gemm.h).  DenseSolver::factor() and the diagnostic entry PogsAmdGramCheck both go through gram_product, so what the
// entry reports is what a solve computes.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "common.h"
#include "gemm.h"

namespace pogs_amd {

// What gram_product chose (PogsAmdGramCheck hands it to the caller as eight ints, in this order).
struct GramInfo {
  int path = 0;        // 0: native fp32 / fp64 MFMA product, 1: fp16 split
  int tile = 128;      // workgroup tile
  int ksplit = 1;      // native: K ranges (1: one launch straight into G)
  int kchunk = 0;      // native, ksplit > 1: rows per K range
  int kacc = 0;        // native: rows per inner chunk of the two-level accumulation (0: one level)
  int units = 1;       // K units in all: ksplit, or the units of the fp16 split
  int unit_rows = 0;   // rows per unit
  int tile_map = 0;    // 1: the tiles ran in gram_tile_order
};

// `force`: 0 as the environment says (POGS_AMD_GRAM, POGS_AMD_GRAM_TILE), else what those variables would say --
// kGramForceNative = POGS_AMD_GRAM=fp32, 128 / 256 = POGS_AMD_GRAM_TILE (which, like the variable, only picks the
// tile where the fp16 split is the product of the shape).
constexpr int kGramForceNative = 1;

// G (k x ld, the first of four slabs of k * ld elements, all zero on entry) = P^T P on the lower 128-tiles; the other
// three slabs are scratch and zero again on return.  P: kdim rows of k (leading dimension lda, K-major: the stored rows
// are the K index) or, with kmajor false, k rows of kdim.  amax: the largest |entry| of P (scales the fp16 split).
// host: stream, sync() and tmark(label) -- the solver's Ctx, or a stand-in with the same three members.
template <typename T, typename Host>
GramInfo gram_product(const T *A, size_t lda, int kdim, int k, bool kmajor, double amax, int num_cu, T *G, size_t ld,
                      int force, Host &host) {
  hipStream_t s = host.stream;
  const size_t slab = static_cast<size_t>(k) * ld;
  GramInfo info;
  // split-K: short K ranges keep the workgroups of an XCD in step on the same rows of A
  // (L2 hits; one long K range per tile measured 121 ms against 100 ms at C2), give every
  // CU work to the end of the launch, and form the fp32 K-sum as an ordered sum of short
  // sums: a sequential fp32 sum over 1e5 rows costs ~30 % more ADMM iterations at C2.
  // The K ranges are processed in rounds that write their partial products into the four
  // slabs themselves (4 ranges in the first round, 3 in the later ones: slab 0 carries
  // the running sum), added in range order -- no transient multi-GB allocation, whose
  // first-touch cost was seen to stall this phase by 100-180 ms now and then.
  const long long tiles = static_cast<long long>((k + 127) / 128) * ((k + 127) / 128 + 1) / 2;
  int ksplit = 1;
  while (ksplit < 32 && kdim / (ksplit * 2) >= 2048 && (kdim / ksplit > 6400 || tiles * ksplit < 16LL * num_cu * 3))
    ksplit *= 2;
  GemmArgs<T> g{k, k, kdim, A, lda, A, lda, G, ld, static_cast<T>(1), static_cast<T>(0)};
  g.kchunk = ksplit > 1 ? static_cast<int>(round_up((kdim + ksplit - 1) / ksplit, 32)) : 0;
  g.csplit_stride = slab;
  // where K ranges stay longer than ~6.4k rows the unit itself sums in chunks
  const int klen = ksplit > 1 ? g.kchunk : kdim;
  const int nacc = (klen + 6399) / 6400;
  // (fp32 only: the chunks bound the rounding of a long fp32 sum; an fp64 sum over 1e5 rows is exact to 1e-11,
  // and the one-level kernel runs two workgroups per CU where the two-level one has registers for one)
  g.kacc = (nacc > 1 && std::is_same<T, float>::value) ? static_cast<int>(round_up((klen + nacc - 1) / nacc, 32)) : 0;
  DevBuf<int> tmap;
  if (k > 16 * 128 && k < 65536 * 128) {
    const std::vector<int> order = gram_tile_order(k);
    tmap.alloc(order.size());
    POGS_HIP_CHECK(hipMemcpyAsync(tmap.p, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, s));
    host.sync();   // order is a host temporary
    g.tile_map = tmap.p;
  }
  // fp32, K-major operand, enough rows: the fp16 matrix cores at (better than) fp32 accuracy --
  // operands scaled by a power of two into fp16 range and split in two fp16 parts, three
  // products (gemm.h).  1024-row K ranges, four at a time into the four slabs, each launch
  // adding to what the slabs hold; then the slabs are added in order.
  const char *gsel = force == 0 ? std::getenv("POGS_AMD_GRAM") : (force == kGramForceNative ? "fp32" : nullptr);
  bool split16 = std::is_same<T, float>::value && kmajor && kdim >= 8192 && k >= 256 &&
                 !(gsel && gsel[0] == 'f') && std::isfinite(amax) && amax > 0;
  float scale16 = 1.f;
  if (split16) {
    int ex = 0;
    std::frexp(amax, &ex);                        // amax = f * 2^ex, f in [0.5, 1)
    scale16 = std::ldexp(1.f, 14 - ex);           // largest scaled entry in [8192, 16384)
    split16 = std::isfinite(scale16) && scale16 > 0;
  }
  if (split16) {
    // The K dimension is cut into equal units of at most ~12800 rows, four per launch into the
    // four slabs (C2: 2 launches x 4 units of 12512 rows): long units pay the accumulator
    // read-add-write, the prologue and the first-copy latency less often, equal ones leave no
    // mostly-empty unit at the end.  The rows of a launch are first written as two fp16 images
    // in operand order (launch_split_f16: 168 MB per 4096 rows at C2), which the product kernel
    // copies straight into LDS (gemm.h).
    // 256 x 256 workgroup tiles (half the operand bytes per product of the 128 tile; one
    // accumulator set, i.e. a unit is ONE MFMA chain -- chains of 1024 .. 16384 rows give the same
    // 106 iterations at C2 and x within 6e-7 of each other, the distance the native fp32 product
    // is at) from n = 4096 on; the 128 tile below, with
    // 1024-row chains added to a second register set.  POGS_AMD_GRAM_TILE=128 forces the 128
    // tile (regression sweep of tests/test_gpu_dense.py).
    constexpr int kRows = 1024, kUnitCap = 12800;
    const int launches = (kdim + 4 * kUnitCap - 1) / (4 * kUnitCap);
    // (measured with 200000 rows, phase in ms, 128 | 256 tile: n = 3072 7.5 | 7.9, 4096 12.6 | 12.2, 5000 18.5 | 16.7,
    // 6144 25.9 | 21.8, 7168 34.4 | 30.0)
    int tile = k >= 4096 ? 256 : 128;
    if (force == 128 || force == 256) {
      tile = force;
    } else if (force == 0) {
      if (const char *ev = std::getenv("POGS_AMD_GRAM_TILE")) tile = std::atoi(ev) == 256 ? 256 : 128;
    }
    const int urows = static_cast<int>(round_up(static_cast<size_t>((kdim + 4 * launches - 1) / (4 * launches)), 32));
    const int nunits = (kdim + urows - 1) / urows;
    const int npad = static_cast<int>(round_up(k, tile));
    DevBuf<unsigned char> img(static_cast<size_t>(2) * (4 * urows) * npad * 2);
    unsigned char *H = img.p, *L = img.p + static_cast<size_t>(4 * urows) * npad * 2;
    host.tmark("  gram: images allocated");
    GramF16PArgs gp{H, L, npad, k, reinterpret_cast<float *>(G), ld, 4, urows, slab, 0, g.tile_map, scale16};
    gp.tile = tile;
    gp.flush_rows = kRows;
    DevBuf<int> tmap256;
    if (tile == 256) {
      gp.tile_map = nullptr;
      if (k > 16 * 256) {
        const std::vector<int> order = gram_tile_order(k, 256);
        tmap256.alloc(order.size());
        POGS_HIP_CHECK(hipMemcpyAsync(tmap256.p, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, s));
        host.sync();   // order is a host temporary
        gp.tile_map = tmap256.p;
      }
    }
    for (int u0 = 0; u0 < nunits; u0 += 4) {
      gp.nslabs = std::min(4, nunits - u0);
      gp.accumulate = u0 > 0 ? 1 : 0;
      launch_split_f16(reinterpret_cast<const float *>(A), lda, kdim, k, u0 * urows, gp.nslabs * urows, npad,
                       scale16, H, L, s);
      launch_gram_f16p(gp, s);
    }
    const int nslabs_used = std::min(4, nunits);
    host.sync();   // img is freed at scope exit
    launch_sum_slabs<T>(G, slab, nslabs_used, G, ld, k, s);
    ksplit = 0;   // skip the fp32 rounds below
    POGS_HIP_CHECK(hipMemsetAsync(G + slab, 0, 3 * slab * sizeof(T), s));
    info.path = 1;
    info.ksplit = 0;
    info.tile = tile;
    info.units = nunits;
    info.unit_rows = urows;
    info.tile_map = gp.tile_map != nullptr;
  } else {
    info.ksplit = ksplit;
    info.kchunk = g.kchunk;
    info.kacc = g.kacc;
    info.units = ksplit;
    info.unit_rows = klen;
    info.tile_map = g.tile_map != nullptr;
  }
  for (int ks = 0; ks < ksplit;) {
    const bool first = ks == 0;
    const int nb = std::min(first ? 4 : 3, ksplit - ks);
    g.ks0 = ks;
    g.ksplit = nb;
    g.C = first ? G : G + slab;
    launch_gemm<T>(kmajor, kmajor, true, g, s);   // K-major when the stored rows are the K index
    if (ksplit > 1) launch_sum_slabs<T>(G, slab, first ? nb : nb + 1, G, ld, k, s);   // in place: slab 0 is G
    ks += nb;
  }
  if (ksplit > 1) POGS_HIP_CHECK(hipMemsetAsync(G + slab, 0, 3 * slab * sizeof(T), s));
  host.sync();   // tmap is freed at scope exit
  return info;
}

}  // namespace pogs_amd

#pragma once
// SparseOperator<T>: the sparse matrix of the solo solver as the device sees it -- A and A^T as CSR (validated,
// transposed on the device), their tiled lane-stream copies (sell.h: planned, filled, refilled once the values are
// final), the product launchers on either copy and the per-XCD stamp diagnostic.  It works on a Ctx it is given and
// knows nothing of ADMM, of functions or of row shards; PogsAmdSpmvCheck builds one without a solver.
// Mixed storage (fp64 only): round_values() rounds both CSR copies to float-representable doubles, finalize_values(true)
// then stores the tiled VALUES as floats and every product on a tiled copy runs the S = float kernel of sell.h.
//
// Included by sparse.hip only -- the anonymous namespace keeps every kernel in that translation unit.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "cg_fused.h"
#include "cg_kernels.h"
#include "engine.h"
#include "sell.h"
#include "sparse_kernels.h"
#include "spmv_check.h"
#include "vec_kernels.h"

namespace pogs_amd {
namespace {

// ---------------------------------------------------------------------------
// One-time structure kernels
// ---------------------------------------------------------------------------
// *err |= 1 if ptr decreases somewhere, 2 if an index lies outside [0, ncols): checked before any
// kernel scatters through these arrays (a malformed CSR / CSC is an error return, not a fault)
__global__ void validate_csr_kernel(const int *ind, const int *ptr, int nrows, int ncols, size_t nnz, int *err) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t t0 = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  int bad = 0;
  for (size_t r = t0; r < static_cast<size_t>(nrows); r += stride)
    if (ptr[r + 1] < ptr[r]) bad |= 1;
  for (size_t k = t0; k < nnz; k += stride) {
    const int c = ind[k];
    if (c < 0 || c >= ncols) bad |= 2;
  }
  if (bad) atomicOr(err, bad);
}

__global__ void count_cols_kernel(const int *ind, size_t nnz, int *cnt) {
  for (size_t k = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < nnz;
       k += static_cast<size_t>(gridDim.x) * blockDim.x)
    atomicAdd(&cnt[ind[k]], 1);
}

// exclusive scan of cnt[0..n) into ptr[0..n], single workgroup of 1024 threads
__global__ void __launch_bounds__(1024) scan_kernel(const int *cnt, int n, int *ptr) {
  __shared__ int s_tot[1024];
  const int t = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int lo = t * chunk, hi = min(n, lo + chunk);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  s_tot[t] = sum;
  __syncthreads();
  // Hillis-Steele inclusive scan over the 1024 chunk totals
  for (int off = 1; off < 1024; off <<= 1) {
    int v = (t >= off) ? s_tot[t - off] : 0;
    __syncthreads();
    s_tot[t] += v;
    __syncthreads();
  }
  int run = (t == 0) ? 0 : s_tot[t - 1];
  for (int i = lo; i < hi; ++i) {
    ptr[i] = run;
    run += cnt[i];
  }
  if (t == 1023) ptr[n] = s_tot[1023];
}

// Three-kernel exclusive scan for long arrays: per-tile (8192 items) local scan + tile totals,
// scan_kernel over the totals, then the tile offsets are added.
constexpr int kScanTile = 8192;

__global__ void __launch_bounds__(1024) scan_tiles_kernel(const int *cnt, int n, int *out, int *tile_tot) {
  __shared__ int s_w[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int base = blockIdx.x * kScanTile + t * 8;
  int v[8], sum = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = (base + k < n) ? cnt[base + k] : 0;
    sum += v[k];
  }
  // inclusive scan of the thread sums: within the wave by shuffles, then across the 16 waves
  int inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int woff = 0;
  for (int w = 0; w < wave; ++w) woff += s_w[w];
  int run = woff + inc - sum;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (t == 1023) tile_tot[blockIdx.x] = woff + inc;
}

__global__ void __launch_bounds__(1024) scan_add_kernel(int *out, int n, const int *tile_off, int ntiles) {
  const int base = blockIdx.x * kScanTile + threadIdx.x * 8;
  const int off = tile_off[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (base + k < n) out[base + k] += off;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = tile_off[ntiles];
}

// scatter (row, val) of every non-zero into its column segment (order within a
// segment is fixed afterwards by sort_segments_kernel)
template <typename T>
__global__ void fill_transpose_kernel(const T *val, const int *ind, const int *ptr, int nrows, int *cursor,
                                      T *tval, int *tind) {
  const int lane = threadIdx.x & 63;
  const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  for (int r = w; r < nrows; r += nw) {
    for (int k = ptr[r] + lane; k < ptr[r + 1]; k += 64) {
      const int pos = atomicAdd(&cursor[ind[k]], 1);
      tind[pos] = r;
      tval[pos] = val[k];
    }
  }
}

// Sorts each segment by index with an all-ascending bitonic network, so the transposed matrix is
// exactly what the reference's stable csr2csc builds (gsl_spmat.h:32-55).  An input that repeats
// an entry (the same column twice in a row: the reference's gather product simply adds both,
// gsl_spblas.h:16-40) leaves ties, which the scatter above delivers in no particular order: they
// are broken by the value's bit pattern, so the stored order -- and with it every sum -- is the
// same from run to run (the reference's order among such ties is their CSR order; the two differ
// only in the association of three or more equal-index terms).  One workgroup per segment; LDS
// when it fits.
template <typename T>
__global__ void __launch_bounds__(256) sort_segments_kernel(const int *ptr, int nseg, int *ind, T *val) {
  constexpr int CAP = 2048;
  __shared__ int s_i[CAP];
  __shared__ T s_v[CAP];
  for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    const int p0 = ptr[seg], len = ptr[seg + 1] - p0;
    if (len <= 1) continue;
    const bool lds = len <= CAP;
    int *ki = lds ? s_i : ind + p0;
    T *kv = lds ? s_v : val + p0;
    if (lds) {
      for (int k = threadIdx.x; k < len; k += 256) { s_i[k] = ind[p0 + k]; s_v[k] = val[p0 + k]; }
    }
    __syncthreads();
    int np2 = 1;
    while (np2 < len) np2 <<= 1;
    for (int k = 2; k <= np2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < np2; i += 256) {
          const int l = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);
          if (l > i && l < len) {  // elements >= len act as +inf and never move
            const int a = ki[i], b = ki[l];
            const T va = kv[i], vb = kv[l];
            bool swap = a > b;
            if (a == b) {
              typename std::conditional<sizeof(T) == 4, unsigned, unsigned long long>::type ba, bb;
              __builtin_memcpy(&ba, &va, sizeof(T));
              __builtin_memcpy(&bb, &vb, sizeof(T));
              swap = ba > bb;
            }
            if (swap) {
              ki[i] = b; ki[l] = a;
              kv[i] = vb; kv[l] = va;
            }
          }
        }
        __syncthreads();
      }
    }
    if (lds) {
      for (int k = threadIdx.x; k < len; k += 256) { ind[p0 + k] = s_i[k]; val[p0 + k] = s_v[k]; }
    }
    __syncthreads();
  }
}

// val <- (double)(float) val, to nearest: the rounding of a mixed-storage handle (PogsAmdCreateSparseMixed).  Both CSR
// copies hold bitwise-equal values when it runs (scale_csr_kernel: a commutative product), so they stay equal.
__global__ void round_to_f32_kernel(double *val, size_t nnz) {
  for (size_t k = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < nnz;
       k += static_cast<size_t>(gridDim.x) * blockDim.x)
    val[k] = static_cast<double>(static_cast<float>(val[k]));
}

// ---------------------------------------------------------------------------
template <typename T>
struct DevCsr {
  DevBuf<T> val;
  DevBuf<int> ind, ptr, blocks;
  int nrows = 0, ncols = 0, nblocks = 0;
  size_t nnz = 0;
  Csr<T> view() const { return Csr<T>{val.p, ind.p, ptr.p, blocks.p, nrows, nblocks}; }
  // tiled lane-stream copy (sell.h); sell_ready == false: not built, the plain kernel runs
  DevBuf<T> sval, part;
  DevBuf<float> sval32;          // mixed storage (T = double): the tiled values as floats, INSTEAD of sval (finalize_values)
  bool mixed = false;            // the tiled copy's values are sval32: every product runs the S = float kernel
  DevBuf<unsigned short> sloc, srid;
  DevBuf<int> tile_unit;
  DevBuf<unsigned short> scnt;   // build temporaries kept until the values are final (refill_sell)
  DevBuf<unsigned> ssoff;
  DevBuf<unsigned> sdst;         // position of every CSR element in the tiled copy, kept from the first fill to the refill
  bool sell_ready = false;
  int sell_why = kSellWhyNone;   // why the plain kernel runs instead (sell.h: kSellWhy*), kSellWhyNone on a tiled copy
  int rr_rows = 0, nrr = 0, ncb = 0, ncg = 1;
  int two = 0;                   // storage format (SellView::two)
  size_t sell_elems = 0;
  DevBuf<unsigned long long> stamps;      // debug time stamps (POGS_AMD_SELL_STAMPS)
  bool stamps_on = false;
  SellDims sdims() const { return SellDims{nrows, ncols, rr_rows, nrr, ncb, SellCfg<T>::BW}; }
  SellView<T> sview() const {
    return SellView<T>{sval.p, sloc.p, srid.p, tile_unit.p, nrows, ncols, rr_rows, nrr, ncb, ncg, two,
                       stamps_on ? stamps.p : nullptr};
  }
  SellView<T, float> sview32() const {
    return SellView<T, float>{sval32.p, sloc.p, srid.p, tile_unit.p, nrows, ncols, rr_rows, nrr, ncb, ncg, two,
                              stamps_on ? stamps.p : nullptr};
  }
};

std::vector<int> make_row_blocks(const std::vector<int> &ptr, int nrows) {
  std::vector<int> blocks;
  blocks.push_back(0);
  int start = 0;
  while (start < nrows) {
    int end = start;
    long long cnt = 0;
    while (end < nrows && end - start < kSpMaxRows) {
      const long long rn = ptr[end + 1] - ptr[end];
      if (cnt + rn > kSpCap) break;
      cnt += rn;
      ++end;
    }
    if (end == start) ++end;  // a single row longer than a tile
    blocks.push_back(end);
    start = end;
  }
  return blocks;
}

// What PogsAmdSpmvCheck pins and a solve leaves alone (the defaults: as a solve chooses)
struct SpmvChoice {
  int format = kSpmvFormatAuto;   // kSpmvFormat* (spmv_check.h); Auto consults POGS_AMD_SPMV / POGS_AMD_SELL_FORMAT
  int rr_rows = 0, ncg = 0;       // row-range height and column-group count of copy `copy`, where not 0
  int copy = -1;                  // 0: A, 1: A^T
};

template <typename T>
class SparseOperator {
 public:
  // val / ptr / ind: CSR (ROW_MAJ) or CSC of the m x n matrix, on the host or the device (`mem`)
  SparseOperator(Ctx &ctx, int ord, int m, int n, size_t nnz, const void *val, const int *ptr, const int *ind, int mem,
                 const SpmvChoice &choice = SpmvChoice{})
      : ctx_(ctx), m_(m), n_(n), nnz_(nnz), choice_(choice), grid_cap_(ctx.num_cu * 8) {
    // an explicit format wins; Auto reads the environment's switches: POGS_AMD_SPMV=plain keeps the plain CSR kernel
    // (testing aid), POGS_AMD_SELL_FORMAT=tags / two pins the storage format (tests, A/B measurements)
    const bool env = choice.format == kSpmvFormatAuto;
    const char *ev = std::getenv("POGS_AMD_SPMV"), *ef = std::getenv("POGS_AMD_SELL_FORMAT");
    plain_ = choice.format == kSpmvFormatPlain || (env && ev && ev[0] == 'p');
    if (choice.format == kSpmvFormatTags) want_two_ = 0;
    else if (choice.format == kSpmvFormatTwo) want_two_ = 1;
    else if (env && ef) want_two_ = std::strcmp(ef, "two") == 0 ? 1 : (std::strcmp(ef, "tags") == 0 ? 0 : -1);
    build_structure(ord, val, ptr, ind, mem);
  }

  const DevCsr<T> &A() const { return A_; }
  const DevCsr<T> &At() const { return At_; }
  bool first_is_A() const { return first_is_A_; }   // the caller's copy is A (CSR input); the other was transposed here
  int grid_cap() const { return grid_cap_; }        // workgroups of a grid-stride launch over rows
  // workgroups that write scalar partials (ctx.spart) in one launch
  size_t partials_needed() const {
    size_t sg = static_cast<size_t>(grid_cap_);
    if (A_.sell_ready) sg = std::max(sg, static_cast<size_t>(A_.nrr) * A_.ncg);
    if (At_.sell_ready) sg = std::max(sg, static_cast<size_t>(At_.nrr) * At_.ncg);
    return sg;
  }

  // val <- D val E on both CSR copies (d: m row factors, e: n column factors); each launch leaves grid_cap()
  // partial sums of the squared new values, A's in partials_a, A^T's in partials_at
  void scale(const T *d, const T *e, double *partials_a, double *partials_at) {
    hipStream_t s = ctx_.stream;
    const int g = grid_cap_;
    hipLaunchKernelGGL(scale_csr_kernel<T>, dim3(g), dim3(256), 0, s, A_.val.p, A_.ind.p, A_.ptr.p, m_, d, e, partials_a);
    hipLaunchKernelGGL(scale_csr_kernel<T>, dim3(g), dim3(256), 0, s, At_.val.p, At_.ind.p, At_.ptr.p, n_, e, d,
                       partials_at);
  }
  void scal(T alpha) {
    launch_scal<T>(A_.val.p, alpha, nnz_, ctx_.stream);
    launch_scal<T>(At_.val.p, alpha, nnz_, ctx_.stream);
  }
  // Mixed storage: every value of both CSR copies rounded to the nearest float, kept as that double.  Called once the
  // values are final, just before finalize_values(): everything after it is defined on the rounded matrix.
  void round_values() {
    if constexpr (std::is_same<T, double>::value) {
      if (!nnz_) return;
      const int g = static_cast<int>(std::min<size_t>((nnz_ + 255) / 256, static_cast<size_t>(ctx_.num_cu) * 32));
      hipLaunchKernelGGL(round_to_f32_kernel, dim3(g), dim3(256), 0, ctx_.stream, A_.val.p, nnz_);
      hipLaunchKernelGGL(round_to_f32_kernel, dim3(g), dim3(256), 0, ctx_.stream, At_.val.p, nnz_);
    } else {
      throw Error("mixed storage needs an fp64 operator");
    }
  }
  // the CSR values are final: the tiled copies take them and the build temporaries go.  as_float (mixed storage, after
  // round_values): the tiled values are written as floats -- the fp64 arrays are released first -- and every product
  // on a tiled copy runs the S = float kernel from here on; loc, rid, tile_unit and the plan are untouched.
  void finalize_values(bool as_float = false) {
    refill_sell(A_, as_float);
    refill_sell(At_, as_float);
  }

  // y_i = op(sum_k val * x[ind]) over the rows of M; scalar sums land in S[slot..slot+NS)
  // cg_mode != 0 (single GPU): the scalar sum and the CGLS scalar that consumes it (block `cg`) run as one launch
  template <bool SQ, typename Op>
  void spmv(const DevCsr<T> &M, const T *x, const double *x_nrm2, const Op &op, double *scalar_out, bool timed = false,
            int cg_mode = 0, double *cg = nullptr) {
    hipStream_t s = ctx_.stream;
    int grid;
    if (timed) ctx_.stream_timer.begin(s);
    if (M.sell_ready) {
      if (M.mixed) {
        if constexpr (!SQ && std::is_same<T, double>::value) grid = launch_sell<false, float>(M, M.sview32(), x, x_nrm2, op);
        else throw Error("the mixed tiled copy has no squared product");
      } else {
        grid = launch_sell<SQ, T>(M, M.sview(), x, x_nrm2, op);
      }
    } else {
      grid = std::max(1, std::min(M.nblocks, grid_cap_));
      hipLaunchKernelGGL((spmv_kernel<T, SQ, Op>), dim3(grid), dim3(kSpTpb), 0, s, M.view(), x, x_nrm2, op,
                         ctx_.spart.p);
    }
    if (timed) ctx_.stream_timer.end(s);
    if (Op::NS > 0 && scalar_out) {
      SumJob j{ctx_.spart.p, grid, Op::NS, scalar_out};
      if (cg_mode != 0) launch_sum_cg(j, ctx_.S.p, cg, cg_mode, 1.0, std::numeric_limits<T>::epsilon(), s);
      else launch_sum_jobs(&j, 1, s);
    }
  }
  // A product of the device-resident CG loop (cg_fused.h): the SpMV and, with more than one column
  // group, the group reduction that runs the row functor; both return at once unless the loop's
  // done flag says `run_if_done` (-1: always run).  The functor's scalar records (one per block)
  // go to `rec`; returns how many there are.  *ev: index of the stream-timer pair.
  template <typename Op>
  int spmv_cg(const DevCsr<T> &M, const T *x, const Op &op, double *rec, int run_if_done, size_t *ev) {
    if (M.mixed) {
      if constexpr (std::is_same<T, double>::value) return launch_sell_cg<float>(M, M.sview32(), x, op, rec, run_if_done, ev);
      else throw Error("mixed storage needs an fp64 operator");
    }
    return launch_sell_cg<T>(M, M.sview(), x, op, rec, run_if_done, ev);
  }

  // the eight info words of PogsAmdSpmvCheck for copy c (0: A, 1: A^T)
  void describe(int c, int out[8]) const {
    const DevCsr<T> &C = c ? At_ : A_;
    out[0] = C.sell_ready ? 1 : 0;
    out[1] = C.sell_ready ? C.two : 0;
    out[2] = C.sell_ready ? C.rr_rows : 0;
    out[3] = C.sell_ready ? C.nrr : 0;
    out[4] = C.sell_ready ? C.ncb : 0;
    out[5] = C.sell_ready ? C.ncg : 0;
    out[6] = static_cast<int>(C.sell_elems / 64);
    out[7] = C.sell_why;
  }

  // POGS_AMD_SELL_STAMPS=1 (diagnostic): per-XCD times of both SpMVs on stderr once per handle (sell.h: what they showed).
  void print_stamps() {
    const char *st = std::getenv("POGS_AMD_SELL_STAMPS");
    if (!(st && st[0] == '1')) return;
    DevBuf<T> vin(static_cast<size_t>(std::max(m_, n_))), vout(static_cast<size_t>(std::max(m_, n_)));
    launch_fill<T>(vin.p, static_cast<T>(1), vin.n, ctx_.stream);
    for (DevCsr<T> *M : {&A_, &At_}) {
      if (!M->sell_ready) continue;
      double r[kNumXcd];
      measure_xcd_rates(*M, vin.p, vout.p, 3, r, true);
    }
    ctx_.sync();
  }

 private:
  // ---- the tiled kernel's launches, for either storage type S of the values (sell.h) -----------------------------
  // the product proper (and, with column groups, the reduction that runs the row functor); returns the number of
  // workgroups that left scalar partials in ctx_.spart
  template <bool SQ, typename S, typename Op>
  int launch_sell(const DevCsr<T> &M, const SellView<T, S> &V, const T *x, const double *x_nrm2, const Op &op) {
    hipStream_t s = ctx_.stream;
    constexpr size_t smem = sell_lds_bytes<T>();
    const int g1 = M.nrr * M.ncg;
    if (M.ncg == 1) {
      static SmemGrants grants;
      ensure_dynamic_smem(reinterpret_cast<const void *>(&spmv_sell_kernel<T, SQ, true, Op, S>), smem, grants);
      hipLaunchKernelGGL((spmv_sell_kernel<T, SQ, true, Op, S>), dim3(g1), dim3(kSellTpb), smem, s, V, x, x_nrm2, op,
                         static_cast<T *>(nullptr), ctx_.spart.p, static_cast<const double *>(nullptr));
      return g1;
    }
    static SmemGrants grants;
    ensure_dynamic_smem(reinterpret_cast<const void *>(&spmv_sell_kernel<T, SQ, false, Op, S>), smem, grants);
    hipLaunchKernelGGL((spmv_sell_kernel<T, SQ, false, Op, S>), dim3(g1), dim3(kSellTpb), smem, s, V, x, x_nrm2, op,
                       M.part.p, ctx_.spart.p, static_cast<const double *>(nullptr));
    const int grid = std::max(1, std::min((M.nrows + 255) / 256, grid_cap_));
    hipLaunchKernelGGL((reduce_parts_kernel<T, Op>), dim3(grid), dim3(256), 0, s, M.part.p, M.nrows, M.ncg, op,
                       ctx_.spart.p);
    return grid;
  }
  // the same for a product of the device-resident CG loop (spmv_cg)
  template <typename S, typename Op>
  int launch_sell_cg(const DevCsr<T> &M, const SellView<T, S> &V, const T *x, const Op &op, double *rec, int run_if_done,
                     size_t *ev) {
    hipStream_t s = ctx_.stream;
    constexpr size_t smem = sell_lds_bytes<T>();
    const double *S0 = ctx_.S.p;
    const double *guard = run_if_done == 0 ? S0 + kFcDone : nullptr;
    const int g1 = M.nrr * M.ncg;
    int nrec;
    *ev = ctx_.stream_timer.begin(s);
    if (M.ncg == 1) {
      static SmemGrants grants;
      ensure_dynamic_smem(reinterpret_cast<const void *>(&spmv_sell_kernel<T, false, true, Op, S>), smem, grants);
      hipLaunchKernelGGL((spmv_sell_kernel<T, false, true, Op, S>), dim3(g1), dim3(kSellTpb), smem, s, V, x,
                         static_cast<const double *>(nullptr), op, static_cast<T *>(nullptr), rec, guard);
      nrec = g1;
    } else {
      static SmemGrants grants;
      ensure_dynamic_smem(reinterpret_cast<const void *>(&spmv_sell_kernel<T, false, false, Op, S>), smem, grants);
      hipLaunchKernelGGL((spmv_sell_kernel<T, false, false, Op, S>), dim3(g1), dim3(kSellTpb), smem, s, V, x,
                         static_cast<const double *>(nullptr), op, M.part.p, rec, guard);
      nrec = cgf_blocks(M.nrows);
      hipLaunchKernelGGL((cgf_reduce_kernel<T, Op>), dim3(nrec), dim3(kCgfTpb), 0, s, M.part.p, M.nrows, M.ncg, op, rec, S0,
                         run_if_done);
    }
    ctx_.stream_timer.end(s);
    return nrec;
  }

  // ---- build ---------------------------------------------------------------
  void build_structure(int ord, const void *data, const int *ptr, const int *ind, int mem) {
    hipStream_t s = ctx_.stream;
    // "first" copy = what the caller gave (CSR if ROW_MAJ, CSC = CSR of A^T otherwise)
    const int r1 = (ord == ROW_MAJ) ? m_ : n_, c1 = (ord == ROW_MAJ) ? n_ : m_;
    DevCsr<T> first, second;
    first.nrows = r1;
    second.nrows = c1;
    first.nnz = second.nnz = nnz_;
    const hipMemcpyKind kind = (mem == POGS_AMD_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    first.val.alloc(nnz_); first.ind.alloc(nnz_); first.ptr.alloc(r1 + 1);
    POGS_HIP_CHECK(hipMemcpyAsync(first.val.p, data, nnz_ * sizeof(T), kind, s));
    POGS_HIP_CHECK(hipMemcpyAsync(first.ind.p, ind, nnz_ * sizeof(int), kind, s));
    POGS_HIP_CHECK(hipMemcpyAsync(first.ptr.p, ptr, (r1 + 1) * sizeof(int), kind, s));
    std::vector<int> hptr(r1 + 1);
    if (mem == POGS_AMD_DEVICE) {
      POGS_HIP_CHECK(hipMemcpyAsync(hptr.data(), ptr, (r1 + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
      ctx_.sync();
    } else {
      std::memcpy(hptr.data(), ptr, (r1 + 1) * sizeof(int));
    }
    POGS_CHECK(hptr[0] == 0 && static_cast<size_t>(hptr[r1]) == nnz_, "ptr does not match nnz");
    {
      DevBuf<int> err(1);
      err.zero(s);
      hipLaunchKernelGGL(validate_csr_kernel, dim3(2048), dim3(256), 0, s, first.ind.p, first.ptr.p, r1, c1, nnz_, err.p);
      int herr = 0;
      POGS_HIP_CHECK(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, s));
      ctx_.sync();
      POGS_CHECK((herr & 1) == 0, "sparse matrix: ptr is not non-decreasing");
      POGS_CHECK((herr & 2) == 0, "sparse matrix: an index lies outside [0, columns)");
    }
    // transpose on the device (gsl_spmat.h:32-55)
    second.val.alloc(nnz_); second.ind.alloc(nnz_); second.ptr.alloc(c1 + 1);
    DevBuf<int> cnt(c1 + 1), cursor(c1 + 1);
    cnt.zero(s);
    if (nnz_) hipLaunchKernelGGL(count_cols_kernel, dim3(2048), dim3(256), 0, s, first.ind.p, nnz_, cnt.p);
    exclusive_scan(cnt.p, c1, second.ptr.p);
    POGS_HIP_CHECK(hipMemcpyAsync(cursor.p, second.ptr.p, (c1 + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(fill_transpose_kernel<T>, dim3(2048), dim3(256), 0, s, first.val.p, first.ind.p, first.ptr.p,
                       r1, cursor.p, second.val.p, second.ind.p);
    hipLaunchKernelGGL(sort_segments_kernel<T>, dim3(std::min(c1, 65536)), dim3(256), 0, s, second.ptr.p, c1,
                       second.ind.p, second.val.p);
    first.ncols = c1;
    second.ncols = r1;
    if (!plain_) {
      const int first_copy = (ord == ROW_MAJ) ? 0 : 1;   // 0: A, 1: A^T
      build_sell(first, choice_.copy == first_copy);
      build_sell(second, choice_.copy == 1 - first_copy);
    } else {
      first.sell_why = second.sell_why = kSellWhyPinned;
    }
    // row blocks of the plain CSR kernel: only for a copy that did not get its tiled form (the host
    // walk over every row and the copy of the transposed ptr array cost ~5 ms at C4)
    auto set_blocks = [&](DevCsr<T> &M, const std::vector<int> &hp) {
      std::vector<int> b = make_row_blocks(hp, M.nrows);
      M.nblocks = static_cast<int>(b.size()) - 1;
      M.blocks.alloc(b.size());
      POGS_HIP_CHECK(hipMemcpy(M.blocks.p, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice));
    };
    if (!first.sell_ready) set_blocks(first, hptr);
    if (!second.sell_ready) {
      std::vector<int> hptr2(c1 + 1);
      POGS_HIP_CHECK(hipMemcpyAsync(hptr2.data(), second.ptr.p, (c1 + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
      ctx_.sync();
      set_blocks(second, hptr2);
    }
    if (ord == ROW_MAJ) { A_ = std::move(first); At_ = std::move(second); }
    else { At_ = std::move(first); A_ = std::move(second); }
    first_is_A_ = (ord == ROW_MAJ);
  }

  // ptr[0..n] = exclusive scan of cnt[0..n)
  void exclusive_scan(const int *cnt, int n, int *ptr) {
    hipStream_t s = ctx_.stream;
    if (n <= 4 * kScanTile) {
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, cnt, n, ptr);
      return;
    }
    const int ntiles = (n + kScanTile - 1) / kScanTile;
    DevBuf<int> tot(ntiles), off(ntiles + 1);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(ntiles), dim3(1024), 0, s, cnt, n, ptr, tot.p);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, tot.p, ntiles, off.p);
    hipLaunchKernelGGL(scan_add_kernel, dim3(ntiles), dim3(1024), 0, s, ptr, n, off.p, ntiles);
    ctx_.sync();   // temporaries are freed at scope exit
  }

  // Tiled lane-stream copy of M (sell.h): structure and values now, values again after the
  // equilibration has rescaled the CSR copy (refill_sell).  Skipped (the plain CSR kernel then
  // runs) when the bookkeeping could not be indexed with 32 bits or the padding would blow up.
  // forced (the copy SpmvChoice names): its rr_rows / ncg, where not 0, replace the two choices made below
  void build_sell(DevCsr<T> &M, bool forced = false) {
    hipStream_t s = ctx_.stream;
    constexpr int BW = SellCfg<T>::BW, RRMAX = SellCfg<T>::RR;
    M.sell_why = kSellWhyEmpty;
    if (M.nnz == 0) return;
    const int ncb = (M.ncols + BW - 1) / BW;
    // rows per row range: as many as the LDS holds, fewer when the matrix would otherwise give
    // the chip less than ~2 workgroups per CU (column groups can only multiply by ncb)
    const long long want = static_cast<long long>(M.nrows) * ncb / (2LL * ctx_.num_cu);
    int rr_rows = static_cast<int>(round_up(static_cast<size_t>(std::max<long long>(512, std::min<long long>(RRMAX, want))), 64));
    rr_rows = std::min(rr_rows, RRMAX);
    // column groups: the count that fills whole rounds of workgroups (one per CU) best, with the
    // column blocks split evenly; ties go to fewer groups (fewer partial sums).  How well the launch
    // fills its rounds decides the SpMV time beyond its bytes -- C4, BW x RR -> workgroups -> SpMV:
    // 18432 x 16384 -> 246 (A) / 248 (A^T), one round each -> 152 us; 24576 x 12288 -> 489, two
    // rounds -> 165 us; 22528 x 14336 -> 420, 0.82 of two rounds -> 225 us.  (A joint search over
    // the row-range height and the group count by this fill model alone picked many small groups
    // -- 17 rounds of 28 groups -- and was slower, 250 us: partial sums and per-tile costs are not
    // in the model.  Left at the LDS-limit height.)
    int ncg = 1;
    double best = -1;
    for (int g = 1; g <= std::min(ncb, 32); ++g) {
      const long long nwg = static_cast<long long>((M.nrows + rr_rows - 1) / rr_rows) * g;
      const long long rounds = (nwg + ctx_.num_cu - 1) / ctx_.num_cu;
      const double fill = static_cast<double>(nwg) / static_cast<double>(rounds * ctx_.num_cu);
      const double even = (static_cast<double>(ncb) / g) / static_cast<double>((ncb + g - 1) / g);
      const double eff = fill * even;
      if (eff > best + 1e-9) { best = eff; ncg = g; }
    }
    // Second look with a byte model of ONE workgroup's path (the launch takes rounds x that):
    //   matrix bytes rr * blocks * (nnz per row and block) * 8  +  x slices blocks * BW * s * 0.15 (they
    //   mostly hit L2)  +  partial sums rr * 8 (written, then read by reduce_parts) when there are groups.
    // Candidates are built to fill k rounds of ~250 workgroups exactly: for g groups, nrr = k * 250 / g
    // row ranges of rows / nrr rows each (shorter than the LDS limit).  Calibrated on C4 (forced
    // configurations (round 2, forced through tuning switches since removed): 8128 rows x 1 group +1.9 %, 12288 x 3 +9 %, A^T 8064 x 4
    // +4 %, 16384 x 16 +3 % against the 16384 x 2 / x 8 the rule above picks there); a candidate replaces
    // that choice only when the model sees more than 5 % in it -- matrices whose row count leaves the
    // LDS-limit height with many groups (1.4e6 rows: 14 groups, 1204 workgroups; 4157 GB/s).
    {
      const double d = static_cast<double>(M.nnz) / static_cast<double>(M.nrows) / ncb;
      auto path_bytes = [&](int rr, int g) {
        const long long nwg = static_cast<long long>((M.nrows + rr - 1) / rr) * g;
        const long long rounds = (nwg + ctx_.num_cu - 1) / ctx_.num_cu;
        const double cbg = static_cast<double>((ncb + g - 1) / g);
        return static_cast<double>(rounds) * (rr * cbg * d * 8.0 + cbg * BW * sizeof(T) * 0.15 + (g > 1 ? rr * 8.0 : 0.0));
      };
      const double base = path_bytes(rr_rows, ncg);
      double best_c = base * 0.95;
      const int rr_hi = rr_rows, cap = std::max(1, ctx_.num_cu - 6);
      for (int g = 1; g <= std::min(ncb, 32); ++g)
        for (int k = 1; k <= 8; ++k) {
          const long long nrr_t = static_cast<long long>(k) * cap / g;
          if (nrr_t < 1) continue;
          const int rr = std::max(512, static_cast<int>(round_up(static_cast<size_t>((M.nrows + nrr_t - 1) / nrr_t), 64)));
          if (rr > rr_hi) continue;
          const double c = path_bytes(rr, g);
          if (c < best_c * (1 - 1e-3)) { best_c = c; rr_rows = rr; ncg = g; }
        }
    }
    if (forced && choice_.rr_rows) rr_rows = choice_.rr_rows;
    if (forced && choice_.ncg) ncg = choice_.ncg;
    const int nrr = (M.nrows + rr_rows - 1) / rr_rows;
    const long long ntiles = static_cast<long long>(nrr) * ncb;
    const long long nq = ntiles * rr_rows;
    M.sell_why = kSellWhyPlan;
    if (ntiles >= (1LL << 30) || nq >= (1LL << 31)) return;
    // storage format: the planner lays the tile out both ways and the smaller matrix is kept (7 bytes per stored
    // fp32 element with two id slots per batch, 8 with a tag per element -- but the first needs padding when most
    // rows of a tile hold a single element).  want_two_ (the constructor) pins it.
    static_assert(SellCfg<T>::BW <= 32768, "bit 15 of a local column is the row-end flag of the two-slot format");
    const int want_two = want_two_;
    {
      // The plan keeps 6 bytes per (row, column block) pair (count, stream offset) and 4 more (the second layout's
      // offsets) unless the tag format is pinned -- on a matrix with many column blocks and few non-zeros per row
      // that outweighs the matrix itself (5e6 x 5e6: 272 blocks x 5e6 rows x 10 B = 13.6 GB).  Beyond 4x the CSR
      // bytes, or half of what the device has free, the plain CSR kernel stays (the same exit as a padding blow-up).
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
      const double tmp_bytes = (want_two != 0 ? 10.0 : 6.0) * static_cast<double>(nq);
      const double csr_bytes = static_cast<double>(M.nnz) * (sizeof(T) + 4.0);
      if (tmp_bytes > 4.0 * csr_bytes + 64e6 || (free_b && tmp_bytes > 0.5 * static_cast<double>(free_b))) return;
    }
    M.rr_rows = rr_rows; M.nrr = nrr; M.ncb = ncb; M.ncg = ncg;
    const SellDims D = M.sdims();
    DevBuf<unsigned> soff2;
    M.scnt.alloc(nq); M.ssoff.alloc(nq);
    if (want_two != 0) soff2.alloc(nq);
    M.scnt.zero(s);
    DevBuf<int> nu(ntiles + 1), nu2, err(1);
    err.zero(s);
    const int g = std::max(1, std::min((M.nrows + 3) / 4, ctx_.num_cu * 32));   // a wavefront per row, four per workgroup
    hipLaunchKernelGGL(sell_count_kernel, dim3(g), dim3(256), 0, s, M.ind.p, M.ptr.p, D, M.scnt.p, err.p);
    DevBuf<int> tile_unit2;
    if (soff2.p) { nu2.alloc(ntiles + 1); tile_unit2.alloc(ntiles + 1); }
    M.tile_unit.alloc(ntiles + 1);
    const int gt = static_cast<int>(std::min<long long>(ntiles, ctx_.num_cu * 8));
    {
      static SmemGrants grants;   // (row ranges taller than 23 K rows: static + dynamic LDS of the planner pass 64 KB)
      ensure_dynamic_smem(reinterpret_cast<const void *>(&sell_plan_kernel), sell_plan_lds(rr_rows) + 32768, grants);
    }
    hipLaunchKernelGGL(sell_plan_kernel, dim3(gt), dim3(256), sell_plan_lds(rr_rows), s, M.scnt.p, D, nu.p,
                       M.ssoff.p, nu2.p, soff2.p, err.p);
    exclusive_scan(nu.p, static_cast<int>(ntiles), M.tile_unit.p);
    int tot = 0, tot2 = 0, herr = 0;
    POGS_HIP_CHECK(hipMemcpyAsync(&tot, M.tile_unit.p + ntiles, sizeof(int), hipMemcpyDeviceToHost, s));
    if (soff2.p) {
      exclusive_scan(nu2.p, static_cast<int>(ntiles), tile_unit2.p);
      POGS_HIP_CHECK(hipMemcpyAsync(&tot2, tile_unit2.p + ntiles, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    POGS_HIP_CHECK(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    ctx_.sync();
    M.two = 0;
    if (soff2.p && !(herr & 8) && tot2 > 0) {
      // bytes per stored element: value + local column + (2 ids per 4 | a tag)
      const double b2 = static_cast<double>(tot2) * (sizeof(T) + 3.0), b1 = static_cast<double>(tot) * (sizeof(T) + 4.0);
      if (want_two == 1 || b2 < b1) {
        M.two = 1;
        tot = tot2;
        M.ssoff = std::move(soff2);
        M.tile_unit = std::move(tile_unit2);
      }
    }
    // each layout has its own range check (bit 4: the tag layout's 23-bit stream offsets, bit 8: the two-slot
    // layout's 22-bit ones): only the chosen layout's decides whether the tiled copy is usable
    herr &= M.two ? ~4 : ~8;
    if (std::getenv("POGS_AMD_TRACE"))
      std::fprintf(stderr, "[pogs_amd trace] tiled copy %d x %d: %s, %.3f stored elements per non-zero\n", M.nrows, M.ncols,
                   M.two ? "two id slots per batch" : "a row tag per element",
                   static_cast<double>(tot) * 64.0 / static_cast<double>(M.nnz));
    // (a padding blow-up beyond 4x the non-zeros -- a few very long rows among many short ones in
    // a tile -- is left to the plain kernel)
    // (bit 16, sell_count_kernel: a row holds more non-zeros in one tile than the 16-bit counts of the plan can say --
    // only an input that repeats entries gets there -- and the plan made from the clipped counts must not be filled)
    if (herr != 0 || tot <= 0 || static_cast<size_t>(tot) * 64 > 4 * M.nnz + (static_cast<size_t>(1) << 22)) {
      M.sell_why = (herr & kSellErrCount) ? kSellWhyCount : (herr != 0 ? kSellWhyRange : kSellWhyPadding);
      M.scnt.release(); M.ssoff.release(); M.tile_unit.release();
      return;
    }
    M.sell_why = kSellWhyNone;
    M.sell_elems = static_cast<size_t>(tot) * 64;
    M.sval.alloc(M.sell_elems);
    M.sloc.alloc(M.sell_elems);
    M.srid.alloc(M.two ? M.sell_elems / 2 : M.sell_elems);
    M.sval.zero(s);
    M.sloc.zero(s);
    // (tags: kSellNoRow everywhere but on row ends; two id slots: an unused slot names row 0 -- it is looked up, never written)
    POGS_HIP_CHECK(hipMemsetAsync(M.srid.p, M.two ? 0x00 : 0xFF, M.srid.n * sizeof(unsigned short), s));
    M.sell_ready = true;
    fill_sell(M, true);
    if (ncg > 1) M.part.alloc(static_cast<size_t>(ncg) * M.nrows);
    ctx_.sync();   // nu / err are freed at scope exit
  }

  // (re)writes the tiled values from M.val; with_loc also the local columns and the row tags
  void fill_sell(DevCsr<T> &M, bool with_loc) {
    if (!M.sell_ready) return;
    hipStream_t s = ctx_.stream;
    // the first fill records where every CSR element went (4 B per non-zero until refill_sell): the
    // values are written once more after equilibration, and walking the (row, tile) bookkeeping a
    // second time costs 6.7 ms per copy at C4 against 1 ms for a gather through that table
    if (with_loc && M.sell_elems < (static_cast<size_t>(1) << 32)) M.sdst.alloc(M.nnz);
    const int g = std::max(1, std::min((M.nrows + 3) / 4, ctx_.num_cu * 32));   // a wavefront per row, four per workgroup
    hipLaunchKernelGGL(sell_fill_kernel<T>, dim3(g), dim3(256), 0, s, M.val.p, M.ind.p, M.ptr.p, M.sdims(), M.scnt.p,
                       M.ssoff.p, M.tile_unit.p, M.sval.p, with_loc ? M.sloc.p : nullptr, M.srid.p,
                       with_loc ? M.sdst.p : nullptr, M.two);
    ctx_.sync();
  }
  // the values are final (equilibrated): refill and drop the build temporaries
  void refill_sell(DevCsr<T> &M, bool as_float = false) {
    if (as_float && M.sell_ready) {
      // mixed storage: float values in the same places.  The fp64 array goes first (nothing in flight reads it: the
      // stream is waited for), so the copy's peak does not grow; the padding of the streams stays zero.
      ctx_.sync();
      M.sval.release();
      M.sval32.alloc(M.sell_elems);
      M.sval32.zero(ctx_.stream);
      if (M.sdst.p) {
        const int g = static_cast<int>(std::min<size_t>((M.nnz + 255) / 256, static_cast<size_t>(ctx_.num_cu) * 32));
        hipLaunchKernelGGL((sell_refill_kernel<T, float>), dim3(std::max(1, g)), dim3(256), 0, ctx_.stream, M.val.p,
                           M.sdst.p, M.nnz, M.sval32.p);
      } else {   // (no position table: a copy of 2^32 stored elements or more) the plan is walked again
        const int g = std::max(1, std::min((M.nrows + 3) / 4, ctx_.num_cu * 32));
        hipLaunchKernelGGL((sell_fill_kernel<T, float>), dim3(g), dim3(256), 0, ctx_.stream, M.val.p, M.ind.p, M.ptr.p,
                           M.sdims(), M.scnt.p, M.ssoff.p, M.tile_unit.p, M.sval32.p,
                           static_cast<unsigned short *>(nullptr), M.srid.p, static_cast<unsigned *>(nullptr), M.two);
      }
      ctx_.sync();
      M.mixed = true;
    } else if (M.sell_ready && M.sdst.p) {
      const int g = static_cast<int>(std::min<size_t>((M.nnz + 255) / 256, static_cast<size_t>(ctx_.num_cu) * 32));
      hipLaunchKernelGGL(sell_refill_kernel<T>, dim3(std::max(1, g)), dim3(256), 0, ctx_.stream, M.val.p, M.sdst.p, M.nnz,
                         M.sval.p);
      ctx_.sync();
    } else {
      fill_sell(M, false);
    }
    M.sdst.release();
    M.scnt.release();
    M.ssoff.release();
  }


  // Per-XCD streaming rates from time-stamped launches of M's SpMV (workgroup b: work units / duration,
  // summed per XCC id); `reps` launches after one untimed.  Debug / calibration aid.
  void measure_xcd_rates(DevCsr<T> &M, const T *xin, T *yout, int reps, double *rate, bool print) {
    hipStream_t s = ctx_.stream;
    const int nwg = M.nrr * M.ncg;
    M.stamps.alloc(static_cast<size_t>(nwg) * 4);
    std::vector<unsigned long long> h(static_cast<size_t>(nwg) * 4);
    std::vector<double> work(kNumXcd, 0.0), time(kNumXcd, 0.0), tmax(kNumXcd, 0.0);
    std::vector<int> cnt(kNumXcd, 0);
    double kernel_us = 0;
    for (int r = 0; r <= reps; ++r) {
      M.stamps_on = true;
      spmv<false>(M, xin, nullptr, SpAxpbyOp<T>{1, 0, nullptr, yout}, nullptr);
      M.stamps_on = false;
      POGS_HIP_CHECK(hipMemcpyAsync(h.data(), M.stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      ctx_.sync();
      if (r == 0) continue;
      unsigned long long lo = ~0ull, hi = 0;
      for (int b = 0; b < nwg; ++b) {
        const unsigned long long t0 = h[4 * b], t1 = h[4 * b + 1];
        const int x = static_cast<int>(h[4 * b + 2]) & (kNumXcd - 1);
        const double us = static_cast<double>(t1 - t0) / 100.0;   // wall_clock64: 100 MHz
        work[x] += static_cast<double>(h[4 * b + 3]);
        time[x] += us;
        tmax[x] = std::max(tmax[x], us);
        cnt[x]++;
        lo = std::min(lo, t0);
        hi = std::max(hi, t1);
      }
      kernel_us += static_cast<double>(hi - lo) / 100.0;
    }
    for (int x = 0; x < kNumXcd; ++x) rate[x] = time[x] > 0 ? work[x] / time[x] : 1.0;
    if (print) {
      std::fprintf(stderr, "[pogs_amd stamps] %d x %d, %d workgroups, first start to last end %.1f us; per XCD mean us (max) [rate]:",
                   M.nrows, M.ncols, nwg, kernel_us / reps);
      double rs = 0;
      for (int x = 0; x < kNumXcd; ++x) rs += rate[x];
      for (int x = 0; x < kNumXcd; ++x)
        std::fprintf(stderr, " %.1f (%.1f) [%.3f]", cnt[x] ? time[x] / cnt[x] : 0.0, tmax[x], rate[x] * kNumXcd / rs);
      std::fprintf(stderr, "\n");
    }
  }


  Ctx &ctx_;
  int m_, n_;
  size_t nnz_;
  SpmvChoice choice_;
  int grid_cap_;
  bool plain_ = false;
  int want_two_ = -1;   // storage format: -1 the smaller of the two, 0 a row tag per element, 1 two id slots per batch
  bool first_is_A_ = true;
  DevCsr<T> A_, At_;
};
}  // namespace
}  // namespace pogs_amd

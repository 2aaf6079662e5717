// The sparse solver's direct projector (sparse.hip: SparseSolver with POGS_AMD_PROJ_DIRECT): the kernels that the
// dense factorisation pieces (gemm.h) and the batched row pass (batch_kernels.h) do not supply.
//
//   * sparse Gram product   G = S^T S (lower triangle, dense K x K) from the two equilibrated CSR copies, K = min(m, n):
//                           S = A for m > n (A^T A), S = A^T otherwise (A A^T);
//   * triangular mat-vec    y = tri(M) x for the lower triangle of W = L^-1 and the upper triangle of U = W^T: the two
//                           products that replace the Cholesky solve in every iteration of a solo solve;
//   * the y half of a wide projection: y = y0 + t with the iteration's bookkeeping.
//
// Both big kernels are bit-reproducible: every sum is formed in an order that depends on the stored matrix only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pogs_amd.h"
#include "batch_kernels.h"
#include "common.h"
#include "reduce.h"

namespace pogs_amd {

// ---- sparse Gram product ---------------------------------------------------------------------------------------
// `outer` has K rows, `inner` is its transpose.  Output row i: for every entry (r, v) of row i of outer, every entry
// (j, w) of row r of inner with j <= i adds v w to G[i][j].
//
// A wavefront owns an output row and keeps its sums as doubles in LDS, `window` columns at a time (a row that is
// longer than the window walks its entries once per window), so the LDS need does not depend on K or on the type.
// 64 outer entries are fetched at once (index, value and the two row pointers of the inner row), then the inner rows
// are taken one after the other in chunks of 64 entries.  The copies may hold a column more than once in a row:
// each lane writes its lane id to a tag slot of its column and reads it back; a chunk in which some lane reads
// another lane's id has two entries of one column and is added lane by lane in lane order, every other chunk as
// plain LDS read-modify-writes.  Either way column j receives its addends in the order (position in the outer row,
// position in the inner row): the bytes of G depend on the stored copies alone -- not on the window, the grid or the
// run.  Products of two floats are exact in double; the sums are rounded to T once, when the window is written.
// Every j <= i is written, zeros included; nothing above the diagonal or beyond column K is touched.
constexpr int kSgTpb = 256;                 // 4 wavefronts, a row each
constexpr int kSgWaves = kSgTpb / kWave;
constexpr int kSgWindowAuto = 1024;         // 4 x 1024 x (8 + 2) bytes = 40 KB: four workgroups per CU
constexpr int kSgWindowMax = 2048;
inline size_t sparse_gram_lds_bytes(int window) {
  return static_cast<size_t>(kSgWaves) * window * (sizeof(double) + sizeof(unsigned short));
}

template <typename T>
struct SparseGramArgs {
  const T *oval; const int *oind, *optr;   // outer copy: K rows
  const T *ival; const int *iind, *iptr;   // inner copy: the rows the outer indices name
  int K, window;
  T *G; size_t ldg;
};

template <typename T>
__global__ void __launch_bounds__(kSgTpb) sparse_gram_kernel(SparseGramArgs<T> a) {
  extern __shared__ double sg_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int W = a.window;
  volatile double *acc = sg_lds + static_cast<size_t>(wave) * W;
  volatile unsigned short *tag =
      reinterpret_cast<unsigned short *>(sg_lds + static_cast<size_t>(kSgWaves) * W) + static_cast<size_t>(wave) * W;
  const int nwaves = gridDim.x * kSgWaves;
  for (int i = blockIdx.x * kSgWaves + wave; i < a.K; i += nwaves) {
    const int o0 = a.optr[i], o1 = a.optr[i + 1];
    for (int w0 = 0; w0 <= i; w0 += W) {
      const int wend = min(w0 + W, i + 1);   // columns [w0, wend) of row i
      for (int c = lane; c < wend - w0; c += kWave) acc[c] = 0.0;
      for (int ob = o0; ob < o1; ob += kWave) {
        const int oc = min(kWave, o1 - ob);
        int r = 0, p0 = 0, p1 = 0;
        double v = 0.0;
        if (lane < oc) {
          r = a.oind[ob + lane];
          v = static_cast<double>(a.oval[ob + lane]);
          p0 = a.iptr[r];
          p1 = a.iptr[r + 1];
        }
        for (int e = 0; e < oc; ++e) {
          const double ve = __shfl(v, e, kWave);
          const int q0 = __shfl(p0, e, kWave), q1 = __shfl(p1, e, kWave);
          for (int k0 = q0; k0 < q1; k0 += kWave) {
            const int k = k0 + lane;
            int c = -1;
            double w = 0.0;
            if (k < q1) {
              const int j = a.iind[k];
              if (j >= w0 && j < wend) {
                c = j - w0;
                w = static_cast<double>(a.ival[k]);
              }
            }
            const bool on = c >= 0;
            if (on) tag[c] = static_cast<unsigned short>(lane);
            const bool clash = on && tag[c] != static_cast<unsigned short>(lane);
            if (!__any(clash)) {
              if (on) acc[c] = dev::fma_(ve, w, acc[c]);
            } else {
              unsigned long long todo = __ballot(on);
              while (todo) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1;
                if (lane == l) acc[c] = dev::fma_(ve, w, acc[c]);
              }
            }
          }
        }
      }
      T *row = a.G + static_cast<size_t>(i) * a.ldg + w0;
      for (int c = lane; c < wend - w0; c += kWave) row[c] = static_cast<T>(acc[c]);
    }
  }
}

struct SparseGramInfo {
  int window, windows, grid;
};
// The launch a direct handle's factor runs.  window: 0 (the solver's choice) or a multiple of 64 in [64, kSgWindowMax].
template <typename T>
inline SparseGramInfo launch_sparse_gram(const SparseGramArgs<T> &args, int num_cu, hipStream_t s) {
  SparseGramArgs<T> a = args;
  if (a.window == 0) a.window = std::min(kSgWindowAuto, static_cast<int>(round_up(static_cast<size_t>(a.K), kWave)));
  const size_t smem = sparse_gram_lds_bytes(a.window);
  static SmemGrants grants;
  ensure_dynamic_smem(reinterpret_cast<const void *>(&sparse_gram_kernel<T>), smem, grants);
  const int grid = std::max(1, std::min((a.K + kSgWaves - 1) / kSgWaves, num_cu * 8));
  hipLaunchKernelGGL(sparse_gram_kernel<T>, dim3(grid), dim3(kSgTpb), smem, s, a);
  return SparseGramInfo{a.window, (a.K + a.window - 1) / a.window, grid};
}

// ---- solo triangular mat-vec -------------------------------------------------------------------------------------
// y = tri(M) x, M: n x n row-major with leading dimension ld (a multiple of the 16-byte vector), TRI kTriLower (columns
// 0 .. i of row i) or kTriUpper (columns i .. n - 1).  A wavefront takes row i and then row n - 1 - i, n + 1 entries
// together whatever i, so every wavefront streams the same bytes.  A row is read with 16-byte loads, four in flight
// per lane, over the whole vectors that lie inside the triangle and inside column n; the few entries before the
// first and after the last such vector are read one by one, so nothing outside the triangle and nothing in columns
// n .. ld is ever read.  Each lane adds its products in column order, the 64 partial sums go through the fixed tree
// of dev::wave_sum_valu.
// (the values of stream.h's Tri, which launch_batch_rows takes; stream.h itself does not go with sell.h in one unit)
constexpr int kTriLower = 1, kTriUpper = 2;
constexpr int kTmTpb = 256;
constexpr int kTmWaves = kTmTpb / kWave;
constexpr int kTmU = 4;   // 16-byte loads in flight per lane

template <typename T, int TRI>
__device__ __forceinline__ T tri_row_dot(const T *__restrict__ row, const T *__restrict__ x, int n, int i, int lane) {
  using V = typename Vec16<T>::type;
  constexpr int VEC = Vec16<T>::N;
  const int c0 = TRI == kTriLower ? 0 : i, c1 = TRI == kTriLower ? i + 1 : n;   // columns [c0, c1)
  const int v0 = min(c1, (c0 + VEC - 1) / VEC * VEC);                     // whole vectors: [v0, v1)
  const int v1 = max(v0, c1 / VEC * VEC);
  T acc = 0;
  if (lane < v0 - c0) acc = dev::fma_(row[c0 + lane], x[c0 + lane], acc);
  for (int base = v0; base < v1; base += kWave * VEC * kTmU) {
    V mv[kTmU], xv[kTmU];
#pragma unroll
    for (int u = 0; u < kTmU; ++u) {
      const int c = base + (u * kWave + lane) * VEC;
      T *me = reinterpret_cast<T *>(&mv[u]), *xe = reinterpret_cast<T *>(&xv[u]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) { me[t] = 0; xe[t] = 0; }
      if (c < v1) {
        mv[u] = *reinterpret_cast<const V *>(row + c);
        xv[u] = *reinterpret_cast<const V *>(x + c);
      }
    }
#pragma unroll
    for (int u = 0; u < kTmU; ++u) {
      const T *me = reinterpret_cast<const T *>(&mv[u]), *xe = reinterpret_cast<const T *>(&xv[u]);
#pragma unroll
      for (int t = 0; t < VEC; ++t) acc = dev::fma_(me[t], xe[t], acc);
    }
  }
  if (lane < c1 - v1) acc = dev::fma_(row[v1 + lane], x[v1 + lane], acc);
  return dev::wave_sum_valu(acc);
}

template <typename T, int TRI>
__global__ void __launch_bounds__(kTmTpb) tri_matvec_kernel(const T *__restrict__ M, size_t ld, int n,
                                                           const T *__restrict__ x, T *__restrict__ y) {
  const int lane = threadIdx.x & (kWave - 1);
  const int pair = blockIdx.x * kTmWaves + threadIdx.x / kWave;
  if (pair >= (n + 1) / 2) return;
  const int lo = pair, hi = n - 1 - pair;
  const T a = tri_row_dot<T, TRI>(M + static_cast<size_t>(lo) * ld, x, n, lo, lane);
  if (lane == 0) y[lo] = a;
  if (hi != lo) {
    const T b = tri_row_dot<T, TRI>(M + static_cast<size_t>(hi) * ld, x, n, hi, lane);
    if (lane == 0) y[hi] = b;
  }
}

// x must be 16-byte aligned and hold n elements; y holds n.
template <typename T>
inline void launch_tri_matvec(int tri, const T *M, size_t ld, int n, const T *x, T *y, hipStream_t s) {
  const int grid = ((n + 1) / 2 + kTmWaves - 1) / kTmWaves;
  if (tri == kTriLower) hipLaunchKernelGGL((tri_matvec_kernel<T, kTriLower>), dim3(grid), dim3(kTmTpb), 0, s, M, ld, n, x, y);
  else hipLaunchKernelGGL((tri_matvec_kernel<T, kTriUpper>), dim3(grid), dim3(kTmTpb), 0, s, M, ld, n, x, y);
}

// ---- the y half of a wide projection (projector_direct_dense.cpp:134, then the iteration's bookkeeping) --------------
// ynew = y0 + t ; partial sums of |yprev - ynew|^2 and |y12 - ynew|^2 ; y0 -= ynew        (y0: ytemp)
template <typename T>
__global__ void __launch_bounds__(256) direct_wide_y_kernel(int m, const T *__restrict__ t, const T *__restrict__ yprev,
                                                          const T *__restrict__ y12, T *__restrict__ ytemp,
                                                          T *__restrict__ ynew, double *partials) {
  __shared__ double s_red[2 * (256 / 64)];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (i < m) {
    const T y0 = ytemp[i];
    const T yn = y0 + t[i];
    ynew[i] = yn;
    const T p = yprev[i] - yn, q = y12[i] - yn;
    dev::prod_acc(acc[0], p, p);
    dev::prod_acc(acc[1], q, q);
    ytemp[i] = y0 - yn;
  }
  dev::block_sum<2, 256>(acc, s_red);
  if (threadIdx.x == 0) {
    partials[static_cast<size_t>(blockIdx.x) * 2 + 0] = acc[0];
    partials[static_cast<size_t>(blockIdx.x) * 2 + 1] = acc[1];
  }
}

// ---- the element-wise stage of a wide batched projection -----------------------------------------------------------
// x = x0 - z (z = A^T t, n elements) and y = y0 + t (m elements) for the problems of the slots; one grid row per slot
template <typename T>
__global__ void __launch_bounds__(256) direct_wide_batch_kernel(int n, int m, int bx, size_t ldx, size_t ldy,
                                                              const T *__restrict__ x0, const T *__restrict__ z,
                                                              T *__restrict__ x, const T *__restrict__ y0,
                                                              const T *__restrict__ t, T *__restrict__ y,
                                                              BatchSlots sl) {
  const int p = sl.act[blockIdx.y];
  if (static_cast<int>(blockIdx.x) < bx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t o = static_cast<size_t>(p) * ldx + i;
    if (i < n) x[o] = x0[o] - z[o];
  } else {
    const int i = (blockIdx.x - bx) * 256 + threadIdx.x;
    const size_t o = static_cast<size_t>(p) * ldy + i;
    if (i < m) y[o] = y0[o] + t[o];
  }
}

// Diagnostics behind PogsAmdSparseGramCheck (sparse.hip: it builds a SparseOperator) and PogsAmdTriMatvecCheck (HOST
// arrays; include/pogs_amd.h)
struct SparseGramCheckArgs {
  int dtype, ord, nrows, ncols;
  const int *ptr, *ind;
  const void *val;
  int num_cu, window;
  void *G;
  size_t ldg;
  int *info;
};
void sparse_gram_check(const SparseGramCheckArgs &a);
void tri_matvec_check(int dtype, int tri, int n, const void *M, size_t ldm, const void *x, void *y);

}  // namespace pogs_amd
